// micro_fwd_jvp.inc -- the IDM rollout and kK tangent directions of it in ONE kernel, no tape; included by micro_kernels.hip inside
// namespace dhts, after micro_jvp.inc.
//
// Forward mode walks the steps in the forward's own order, so the blocks of a vehicle-step (e2, e3, l3) are in the forward's registers
// at the moment the tangent sweep wants them, and so is the pre-step (p, v) the parameter partials are recomputed from: neither the
// 12 B tape entry nor the 8 B parameter-tape entry of micro_rollout_fwd_kernel + micro_rollout_jvp_kernel is written or read, and
// nothing of size [T] exists unless the caller asks for hist / t_hist.
//
// Arithmetic: the two kernels' own.  A step forms (dp, dv) by the forward kernel's expressions from the float32 state, calls idm_step,
// and hands MicroTape3{dE[2], dE[3], dLd[3]} to jvp_vehicle (micro_jvp.inc) per direction; kParams calls idm_param_jac once per
// vehicle-step and sums x as micro_rollout_jvp_kernel does (double fused multiply-adds over q = 0 .. 4, then the gap term, then
// (float)(dt cs); +0.f where there is no parameter term).  Nothing is restated but the forward's two lines for (dp, dv): the primal
// outputs are dhts_micro_rollout_fwd's bits and the tangents dhts_micro_rollout_jvp's (tests/test_micro_fwd_jvp_gpu.py).
//
// Layout of a launch: as micro_rollout_jvp_kernel's -- directions [0, n_act) of the pointers it is handed, a slot d >= n_act carries
// zeros and touches no memory.  Every launch of a call recomputes the primal and writes the same p_out, v_out; the host hands hist and
// the forward's fault record to the first launch only.
//   p_in, v_in, p_out, v_out   [L][V] float32      params [6][L][V] double      head [L][2] double
//   t_p_in, t_v_in, t_p_out, t_v_out   [kK][L][V] float32      t_head [kK][L][2] double or NULL      t_params [kK][6][L][V] double
//   hist [T][L][2][V] float32 or NULL (live slots only, as the forward)      t_hist [kK][T][L][2][V] float32 or NULL

// micro_kernels.hip includes this file twice: with DHTS_MICRO_SAMPLES 0 for the kernel described above, then with 1 for its sampled
// form (kSamp), micro_rollout_fwd_jvp_samples_kernel -- siblings from one text, and the first compiles to the code it was before the
// sibling existed (profiles/micro_samples_resources*.txt).
//
// kLead, a template parameter of the SAMPLED form only (dhts_micro_rollout_fwd_jvp_lead): the head vehicle follows a recorded leader,
// MicroLead's lead [T][L][2] float32 and its tangents t_lead [kK][T][L][2] (NULL: zero), as every other vehicle follows the slot in
// front of it; virtual_leader is not called, head / t_head are not read and TH stays zero.  The head's thread owns the leader's slot
// n of S and of TN: it writes row t + 1 there during step t, the row after that in flight in registers.  The head's length tangent
// carries its own share of the gap only, -t_len / 2.  NULL samples and t_samples (both): nothing is observed.  kLead = false is the
// code the sampled form was before (profiles/micro_lead_resources*.txt).
//
// The boundary is three-valued: the template parameter of the sampled form is MicroBoundary kB (micro_kernels.hip), and kHeadGap / kLead /
// kRing below name its values.  kRing (dhts_micro_rollout_fwd_jvp_ring): a ring road -- the head follows the image of the lane's own
// tail one circumference ahead, ((float)((double)p_tail + ring[lane]), v_tail), whose tangents are the tail's state tangents before the
// step.  The TAIL's thread (k == 0) owns slot n of S and of TN: it writes them beside its own stores, before the first barrier and in
// every step; nothing is loaded.  virtual_leader is not called and TH stays zero; the head's length tangent is
// -(t_len[tail] + t_len[head]) / 2, the followers' expression with the tail as its leader.  kB = kBoundHead / kBoundLead are the code
// the form was before (profiles/micro_ring_resources*.txt).

//
// A third pass, DHTS_MICRO_SAMPLES 3, gives the GAUSS-NEWTON form (kGN; dhts_micro_rollout_fwd_jvp_gn),
// micro_rollout_fwd_jvp_gn_kernel<kK, kParams, kB, kBlock>: the normal equations of a trajectory fit instead of samples / t_samples.  At a
// sampled step the thread of a live probe slot forms r = x - target in float32 (NaN = not observed, as the checkpointed target forms)
// and adds the exact double products t_a t_b (a <= b), t_a r and r r of both planes to its own accumulators; after the step loop the
// workgroup sums them over the slots by the target forms' fixed-order pairwise tree in the LDS the loop is done with, and thread 0
// stores sse [L][2], jtr [L][K] and jtj [L][K][K] (both triangles).  No atomics: the same bits every run.  A launch carries the
// directions MicroGn::dir names among the call's K -- every per-direction pointer is the CALL's, not the launch's -- and writes their
// rows of jtr and their pairs of jtj; p_out, v_out, sse NULL: another launch of the call writes them.  Rows of target [T / every][L][2][n]
// travel up to two rows ahead in registers (a row is asked for two sampled steps before its use and copied one before) and are loaded at
// sampled steps only; there is no global store in the step loop.  kBlock is the
// block bound: the accumulators (10 + 4 + 2 doubles at kK = 4) need the registers a block of 1024 does not leave.  Passes 0 and 1 are
// the code they were before (profiles/micro_gn_resources*.txt).

// the direction slot d of a launch carries: its own place among the pointers the launch is handed, or (kGN) gn.dir[d] among the call's
#undef DHTS_GN_DIR
#if DHTS_MICRO_SAMPLES == 3
#define DHTS_GN_DIR(d) gn.dir[d]
#else
#define DHTS_GN_DIR(d) d
#endif
#if !DHTS_MICRO_SAMPLES
__host__ __device__ inline size_t micro_fwd_jvp_lds_bytes(int V, int kK) {
    return sizeof(float2) * (size_t)(2 + 2 * kK) * (size_t)(V + 1) + 2 * sizeof(double) * (size_t)kK;
}
// kGN: what the fit is against, where its sums go and which of the call's n_dir directions this launch carries in its slots
struct MicroGn {
    const float *target;     // [T / every][L][2][n] float32, the layout of samples; NaN = not observed
    double *sse;             // [L][2], or NULL (every launch of a call but the first)
    double *jtr;             // [L][n_dir]
    double *jtj;             // [L][n_dir][n_dir]
    int n_dir;               // K of the call
    int dir[4];              // slot d of the launch carries direction dir[d], d < n_act
};
#endif

// grid = L workgroups (one traffic lane each) of blockDim.x >= V threads (V rounded up to 64): one vehicle per thread, its float32
// (p, v), its kK tangent pairs and its derived parameters in registers for all T steps.  After a step a thread leaves its new (p, v) in
// S [copy][slot] and its new tangents in TN [copy][direction][slot] for its follower -- the head vehicle's thread also leaves the
// tangents of its virtual leader in the slot behind its own (virtual_leader), so every vehicle reads its leader the same way --; the
// copies alternate with the step parity, so a step takes ONE barrier, and that one waits for LDS only: hist / t_hist stores stay in
// flight across it.  The head-gap tangents wait in LDS (TH), as in micro_rollout_jvp_kernel.
// Dynamic LDS: float2 S[2][V + 1] | float2 TN[2][kK][V + 1] | double TH[kK][2]
// err: DHTS_FAULT_COLLISION where idm_step reported one (what the forward kernel reports).  err_jvp: DHTS_FAULT_NAN with the EARLIEST
// (step, vehicle) of the workgroup (what the tangent kernel reports, by the same LDS minimum).  A block smaller than the lane:
// DHTS_FAULT_CAPACITY (index -3) on both records, every output NaN.
// kSamp (micro_rollout_fwd_jvp_samples_kernel): instead of hist / t_hist, row j of samples [T / every][L][2][n] and of each direction of
// t_samples [kK][T / every][L][2][n] takes the probe slots' (p, v) and tangents after step (j + 1) every - 1 -- a thread finds its
// slot's column among the probes once, before the step loop, counts the steps down to the next sampled one and moves running pointers
// from row to row.  samples: live slots only, or NULL (every launch of a call but the first); t_samples: slots at or beyond count 0.
#if !DHTS_MICRO_SAMPLES
template <int kK, bool kParams>
__global__ __launch_bounds__(1024) void micro_rollout_fwd_jvp_kernel(
    int L, int V, int T, double dt, const float *__restrict__ p_in, const float *__restrict__ v_in, const int32_t *__restrict__ count,
    const double *__restrict__ params, const double *__restrict__ head, const float *__restrict__ t_p_in,
    const float *__restrict__ t_v_in, const double *__restrict__ t_head, const double *__restrict__ t_params, int n_act,
    float *__restrict__ p_out, float *__restrict__ v_out, float *__restrict__ t_p_out, float *__restrict__ t_v_out,
    float *__restrict__ hist, float *__restrict__ t_hist, dhts_error *err, dhts_error *err_jvp) {
    constexpr bool kSamp = false, kLead = false, kRing = false, kHeadGap = true, kGN = false;
    constexpr int kBlockBound = 1024;
    const MicroProbes pr = {};
    float *const samples = nullptr, *const t_samples = nullptr;
    const MicroLead ld = {};
#elif DHTS_MICRO_SAMPLES == 3
template <int kK, bool kParams, MicroBoundary kB, int kBlock>
__global__ __launch_bounds__(kBlock) void micro_rollout_fwd_jvp_gn_kernel(
    int L, int V, int T, double dt, const float *__restrict__ p_in, const float *__restrict__ v_in, const int32_t *__restrict__ count,
    const double *__restrict__ params, const double *__restrict__ head, const float *__restrict__ t_p_in,
    const float *__restrict__ t_v_in, const double *__restrict__ t_head, const double *__restrict__ t_params, int n_act,
    float *__restrict__ p_out, float *__restrict__ v_out, float *__restrict__ t_p_out, float *__restrict__ t_v_out,
    MicroProbes pr, MicroGn gn, dhts_error *err, dhts_error *err_jvp, MicroLead ld) {
    constexpr bool kSamp = true, kGN = true, kLead = kB == kBoundLead, kRing = kB == kBoundRing, kHeadGap = kB == kBoundHead;
    constexpr int kBlockBound = kBlock;
    float *const hist = nullptr, *const t_hist = nullptr, *const samples = nullptr, *const t_samples = nullptr;
    static_assert(kK <= 4, "MicroGn::dir has four slots");
#else
template <int kK, bool kParams, MicroBoundary kB>
__global__ __launch_bounds__(1024) void micro_rollout_fwd_jvp_samples_kernel(
    int L, int V, int T, double dt, const float *__restrict__ p_in, const float *__restrict__ v_in, const int32_t *__restrict__ count,
    const double *__restrict__ params, const double *__restrict__ head, const float *__restrict__ t_p_in,
    const float *__restrict__ t_v_in, const double *__restrict__ t_head, const double *__restrict__ t_params, int n_act,
    float *__restrict__ p_out, float *__restrict__ v_out, float *__restrict__ t_p_out, float *__restrict__ t_v_out,
    MicroProbes pr, float *__restrict__ samples, float *__restrict__ t_samples, dhts_error *err, dhts_error *err_jvp, MicroLead ld) {
    constexpr bool kSamp = true, kLead = kB == kBoundLead, kRing = kB == kBoundRing, kHeadGap = kB == kBoundHead, kGN = false;
    constexpr int kBlockBound = 1024;
    float *const hist = nullptr, *const t_hist = nullptr;
#endif
#if DHTS_MICRO_SAMPLES == 3
    // kGN: this vehicle's sums -- sse p, sse v | jtr [kK] | the upper triangle of jtj, row by row
    constexpr int kAcc = 2 + kK + kK * (kK + 1) / 2;
    double acc[kAcc];
#pragma unroll
    for (int i = 0; i < kAcc; ++i) acc[i] = 0.;
#endif
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = blockIdx.x;
    const int k = threadIdx.x;
    const int B = blockDim.x;
    const int P = V + 1;
    float2 *S = reinterpret_cast<float2 *>(lds);         // [copy][P]
    float2 *TN = S + 2 * P;                              // [copy][kK][P]
    double *TH = reinterpret_cast<double *>(TN + 2 * kK * P);      // [kK][2]
    const size_t base = (size_t)lane * V;
    const size_t plane = (size_t)L * V;                  // one direction of a state tangent, one plane of params
    const int nc = count ? count[lane] : V;
    const int n = nc < 0 ? 0 : (nc > V ? V : nc);       // (no slot outside the lane is ever addressed)
    const bool vk = k < n;
    const bool is_head = k == n - 1;
    const int kc = k < V ? k : 0;
    const float dtf = (float)dt;
    const double inv_dt = 1.0 / dt;
    const size_t h_dir = (size_t)T * L * 2 * V;          // one direction of t_hist

#if DHTS_MICRO_SAMPLES == 3
    if constexpr (kGN) {
        if (V > B) {                                     // every output of the lane NaN, the three sums among them
            const float nanf_ = __builtin_nanf("");
            const double nand_ = (double)nanf_;
            if (p_out) for (int i = k; i < V; i += B) { p_out[base + i] = nanf_; v_out[base + i] = nanf_; }
#pragma unroll
            for (int d = 0; d < kK; ++d)
                if (d < n_act)
                    for (int i = k; i < V; i += B) { t_p_out[DHTS_GN_DIR(d) * plane + base + i] = nanf_; t_v_out[DHTS_GN_DIR(d) * plane + base + i] = nanf_; }
            if (k == 0) {
                if (gn.sse) { gn.sse[(size_t)lane * 2] = nand_; gn.sse[(size_t)lane * 2 + 1] = nand_; }
#pragma unroll
                for (int a = 0; a < kK; ++a) {
                    if (a >= n_act) continue;
                    gn.jtr[(size_t)lane * gn.n_dir + DHTS_GN_DIR(a)] = nand_;
#pragma unroll
                    for (int b = 0; b < kK; ++b)
                        if (b < n_act) gn.jtj[((size_t)lane * gn.n_dir + DHTS_GN_DIR(a)) * gn.n_dir + DHTS_GN_DIR(b)] = nand_;
                }
                raise_fault(err, DHTS_FAULT_CAPACITY, 0, lane, -3); raise_fault(err_jvp, DHTS_FAULT_CAPACITY, 0, lane, -3);
            }
            return;
        }
    } else
#endif
    if (V > B) {
        const float nanf_ = __builtin_nanf("");
        for (int i = k; i < V; i += B) { p_out[base + i] = nanf_; v_out[base + i] = nanf_; }
        if (hist)
            for (int s = 0; s < T; ++s)
                for (int i = k; i < 2 * V; i += B) hist[((size_t)s * L + lane) * 2 * V + i] = nanf_;
        for (int d = 0; d < n_act; ++d) {
            for (int i = k; i < V; i += B) { t_p_out[d * plane + base + i] = nanf_; t_v_out[d * plane + base + i] = nanf_; }
            if (t_hist)
                for (int s = 0; s < T; ++s)
                    for (int i = k; i < 2 * V; i += B) t_hist[d * h_dir + ((size_t)s * L + lane) * 2 * V + i] = nanf_;
        }
        if constexpr (kSamp) {
            if (samples) micro_samples_fill(samples, pr, T, L, lane, k, B, nanf_);
            for (int d = 0; d < n_act; ++d)
                if (kHeadGap || t_samples) micro_samples_fill(t_samples + (size_t)d * (T / pr.every) * L * 2 * pr.n, pr, T, L, lane, k, B, nanf_);
        }
        if (k == 0) { raise_fault(err, DHTS_FAULT_CAPACITY, 0, lane, -3); raise_fault(err_jvp, DHTS_FAULT_CAPACITY, 0, lane, -3); }
        return;
    }

    // this thread's vehicle: its state, its tangents, its parameters and their tangents
    float p = p_in[base + kc], v = v_in[base + kc];      // (a slot at or beyond count keeps them: the outputs pass it through)
    float tp[kK], tv[kK];
#pragma unroll
    for (int d = 0; d < kK; ++d) {
        const bool act = vk && d < n_act;
        tp[d] = act ? t_p_in[DHTS_GN_DIR(d) * plane + base + k] : 0.f;
        tv[d] = act ? t_v_in[DHTS_GN_DIR(d) * plane + base + k] : 0.f;
    }
    IdmDerived prm = {};
    IdmParamDerived pm = {};
    double half_len = 0.;
    double tth[kParams ? kK : 1][6];                     // t_theta_0 .. 4, then -(t_len_leader + t_len) / 2
    if constexpr (kParams) {
#pragma unroll
        for (int d = 0; d < kK; ++d)
#pragma unroll
            for (int q = 0; q < 6; ++q) tth[d][q] = 0.;
    }
    if (vk) {
        IdmParams raw;
        raw.a_max = params[0 * plane + base + k]; raw.a_pref = params[1 * plane + base + k];
        raw.v_target = params[2 * plane + base + k]; raw.min_space = params[3 * plane + base + k];
        raw.time_pref = params[4 * plane + base + k]; raw.length = params[5 * plane + base + k];
        prm = idm_derive(raw);
        idm_set_dt(prm, dt);
        const int kl = k + 1 < n ? k + 1 : (kRing ? 0 : k);      // kRing: the head's leader is the tail, its length tangent is live
        half_len = (params[5 * plane + base + kl] + raw.length) * 0.5;
        if constexpr (kLead) { if (is_head && ld.length) half_len = (ld.length[lane] + raw.length) * 0.5; }
        if constexpr (kParams) {
            pm = idm_param_derive(raw);
#pragma unroll
            for (int d = 0; d < kK; ++d) {
                if (d < n_act) {
                    const double *tq = t_params + (size_t)DHTS_GN_DIR(d) * 6 * plane + base;
#pragma unroll
                    for (int q = 0; q < 5; ++q) tth[d][q] = tq[q * plane + k];
                    tth[d][5] = -(tq[5 * plane + kl] + tq[5 * plane + k]) * 0.5;
                    if constexpr (kLead) { if (is_head) tth[d][5] = -tq[5 * plane + k] * 0.5; }      // the leader's length is a constant
                }
            }
        }
    }
    double head_dp = 0., head_dv = 0., ring = 0.;
    if constexpr (kRing) ring = ld.ring[lane];
    else if constexpr (!kLead) { head_dp = head[(size_t)lane * 2]; head_dv = head[(size_t)lane * 2 + 1]; }

    for (int i = k; i < (2 + 2 * kK) * P; i += B) S[i] = make_float2(0.f, 0.f);
    if constexpr (!kHeadGap) { if (k < 2 * kK) TH[k] = 0.; }
#if DHTS_MICRO_SAMPLES == 3
    else if constexpr (kGN) {
        if (k < 2 * kK) {
            int g = gn.dir[0];
#pragma unroll
            for (int d = 1; d < kK; ++d) g = (k >> 1) == d ? gn.dir[d] : g;
            TH[k] = ((k >> 1) < n_act && t_head) ? t_head[((size_t)g * L + lane) * 2 + (k & 1)] : 0.;
        }
    }
#endif
    else if (k < 2 * kK) TH[k] = ((k >> 1) < n_act && t_head) ? t_head[((size_t)(k >> 1) * L + lane) * 2 + (k & 1)] : 0.;
    __syncthreads();

    int fault_step = -1, bad_step = -1;
    if (T > 0) {
        // kLead: the head's thread owns slot n of S and of TN -- row 0 now, row step + 1 during step `step`, the row after that in
        // flight in (lx, ly) and (ltx, lty); a direction of t_lead is T L 2 floats, NULL = zero.  The widest form with the parameter
        // term has no register left for eight more floats (128 VGPRs at 1024 threads): there the tangent rows are loaded in the
        // step that hands them over (kTanAhead false), the state row still travels ahead.
        constexpr bool kTanAhead = !(kParams && kK >= 4) || (kGN && kBlockBound < 1024);
        const float *lrow = nullptr, *ltrow = nullptr;
        float lx = 0.f, ly = 0.f, ltx[kLead && kTanAhead ? kK : 1], lty[kLead && kTanAhead ? kK : 1];
        const size_t lt_dir = (size_t)T * L * 2;
        if (vk) {
            S[k] = make_float2(p, v);
#pragma unroll
            for (int d = 0; d < kK; ++d) {
                TN[d * P + k] = make_float2(tp[d], tv[d]);
                if constexpr (kHeadGap) { if (is_head) TN[d * P + k + 1] = virtual_leader(tp[d], tv[d], TH[2 * d], TH[2 * d + 1]); }
                if constexpr (kRing) { if (k == 0) TN[d * P + n] = make_float2(tp[d], tv[d]); }
            }
            // kRing: the TAIL's thread owns slot n of S and of TN -- its own state one circumference ahead and its own tangents
            if constexpr (kRing) { if (k == 0) S[n] = make_float2((float)((double)p + ring), v); }
            if constexpr (kLead) {
                if (is_head) {
                    lrow = micro_lead_row(ld.lead, lane);
                    ltrow = ld.t_lead ? micro_lead_row(ld.t_lead, lane) : nullptr;
                    S[n] = make_float2(lrow[0], lrow[1]);
#pragma unroll
                    for (int d = 0; d < kK; ++d)
                        TN[d * P + n] = (ltrow && d < n_act) ? make_float2(ltrow[DHTS_GN_DIR(d) * lt_dir], ltrow[DHTS_GN_DIR(d) * lt_dir + 1]) : make_float2(0.f, 0.f);
                    lrow += (size_t)L * 2;
                    if (ltrow) ltrow += (size_t)L * 2;
                    const bool more = T > 1;
                    lx = more ? lrow[0] : 0.f; ly = more ? lrow[1] : 0.f;
                    if constexpr (kTanAhead) {
#pragma unroll
                        for (int d = 0; d < kK; ++d) {
                            const bool on = more && ltrow && d < n_act;
                            ltx[d] = on ? ltrow[DHTS_GN_DIR(d) * lt_dir] : 0.f; lty[d] = on ? ltrow[DHTS_GN_DIR(d) * lt_dir + 1] : 0.f;
                        }
                    }
                }
            }
        }
        __syncthreads();
        // kSamp: this slot's column among the probes, its place `so` in the next row of samples and of direction 0 of t_samples (a row
        // is L 2 n floats, a direction s_dir), and the steps until that row is due
        int col = -1, cd = 0;
        size_t so = 0, s_dir = 0;
        if constexpr (kSamp) {
#if DHTS_MICRO_SAMPLES == 3
            if constexpr (kGN) col = micro_probe_column(pr, k, V);
            else
#endif
            col = (!kHeadGap && t_samples == nullptr) ? -1 : micro_probe_column(pr, k, V);      // kLead, kRing, no sample arrays: no column
            cd = pr.every;
            s_dir = (size_t)(T / pr.every) * L * 2 * pr.n;
            so = (size_t)lane * 2 * pr.n + (col < 0 ? 0 : col);
        }
#if DHTS_MICRO_SAMPLES == 3
        // kGN: this slot's column of the target row to load next (a row is L 2 n floats); the next two sampled rows are in (g1p, g1v) and
        // (g2p, g2v), `rj` rows are behind (the copy g1 = g2 one sampled step after g2's load is where that load is waited for at the
        // latest: one sampled step of cover is certain, two where the compiler renames).  Everything loaded so far arrives here, before the first row is asked for: left pending
        // across the loop's entry, those loads would make every step wait for every load issued since (one counter, in order).
        const float *tg = nullptr;
        float g1p = 0.f, g1v = 0.f, g2p = 0.f, g2v = 0.f;
        int rj = 0;
        const int g_rows = T / pr.every;
        const size_t g_row = (size_t)L * 2 * pr.n;
        const bool g_on = vk && col >= 0;
        if constexpr (kGN) {
            asm volatile("" : "+v"(p), "+v"(v));
#pragma unroll
            for (int d = 0; d < kK; ++d) asm volatile("" : "+v"(tp[d]), "+v"(tv[d]));
            if constexpr (kParams) {
#pragma unroll
                for (int d = 0; d < kK; ++d)
#pragma unroll
                    for (int qq = 0; qq < 6; ++qq) asm volatile("" : "+v"(tth[d][qq]));
            }
            if (g_on && g_rows > 0) {
                tg = gn.target + so;
                g1p = tg[0]; g1v = tg[pr.n];
                tg += g_row;
                if (g_rows > 1) { g2p = tg[0]; g2v = tg[pr.n]; }
            }
        }
#endif
        for (int step = 0; step < T; ++step) {
            const int q = step & 1;
            bool due = false;
            if constexpr (kSamp) { due = --cd == 0; cd = due ? pr.every : cd; }
            if (vk) {
                const float2 ls = S[q * P + k + 1];      // the leader's state before this step
                const double pd = p, vd = v;
                // compute_state_delta, _micro_lane.py:201-212, in the forward kernel's expressions
                const double dp = (kHeadGap && is_head) ? head_dp : fabs((double)ls.x - pd) - half_len;
                const double dv = (kHeadGap && is_head) ? head_dv : vd - (double)ls.y;
                IdmStep o;
                idm_step(pd, vd, dp, dv, prm, dt, inv_dt, o);
                if (o.collided && fault_step < 0) fault_step = step;
                MicroTape3 c;
                c.e2 = o.dE[2]; c.e3 = o.dE[3]; c.l3 = o.dLd[3];
                // kParams: the partials of this vehicle-step, once for all directions (the collision / clamp rules of the forward,
                // _micro_lane.py:149-166, 201-212, as micro_rollout_jvp_kernel rebuilds them from the parameter tape)
                IdmParamJac pj = {};
                bool has_x = false, live_gap = false;
                if constexpr (kParams) {
                    double gap = dp, dvx = dv;
                    live_gap = (!kHeadGap || !is_head) && gap >= 1e-5;      // else a constant: nothing flows to the lengths
                    if (gap < 0) { gap = 0; dvx = 0; }
                    gap = (1e-5 > gap) ? 1e-5 : gap;
                    has_x = !(c.e2 == 0.f && c.e3 == 0.f && c.l3 == 0.f);      // (the forward's acceleration clip zeroes all three)
                    if (has_x) idm_param_jac(vd, gap, dvx, pm, dt, pj);
                }
                bool fin = true;
#pragma unroll
                for (int d = 0; d < kK; ++d) {
                    const float2 tl = TN[(q * kK + d) * P + k + 1];      // the leader's tangents before this step
                    float x = 0.f;
                    if constexpr (kParams) {
                        if (has_x) {
                            double cs = pj.d[0] * tth[d][0];
#pragma unroll
                            for (int qq = 1; qq < 5; ++qq) cs = __builtin_fma(pj.d[qq], tth[d][qq], cs);
                            if (live_gap) cs = __builtin_fma(pj.d[5], tth[d][5], cs);
                            x = (float)(dt * cs);
                        }
                    }
                    float np_, nv_;
                    jvp_vehicle(c, dtf, tp[d], tv[d], tl.x, tl.y, x, np_, nv_);
                    tp[d] = np_; tv[d] = nv_;
                    TN[((q ^ 1) * kK + d) * P + k] = make_float2(np_, nv_);
                    if constexpr (kHeadGap) { if (is_head) TN[((q ^ 1) * kK + d) * P + k + 1] = virtual_leader(np_, nv_, TH[2 * d], TH[2 * d + 1]); }
                    if constexpr (kRing) { if (k == 0) TN[((q ^ 1) * kK + d) * P + n] = make_float2(np_, nv_); }
                    fin = fin && isfinite(np_) && isfinite(nv_);
                }
                if (bad_step < 0 && !fin) bad_step = step;
                p = o.np; v = o.nv;
                S[(q ^ 1) * P + k] = make_float2(p, v);      // what this vehicle enters step + 1 with
                if constexpr (kRing) { if (k == 0) S[(q ^ 1) * P + n] = make_float2((float)((double)p + ring), v); }
                if constexpr (kLead) {
                    if (is_head && step + 1 < T) {           // ... and what its leader is seen at in step + 1, with its tangents
                        S[(q ^ 1) * P + n] = make_float2(lx, ly);
#pragma unroll
                        for (int d = 0; d < kK; ++d) {
                            if constexpr (kTanAhead) TN[((q ^ 1) * kK + d) * P + n] = make_float2(ltx[d], lty[d]);
                            else TN[((q ^ 1) * kK + d) * P + n] = (ltrow && d < n_act) ? make_float2(ltrow[DHTS_GN_DIR(d) * lt_dir], ltrow[DHTS_GN_DIR(d) * lt_dir + 1])
                                                                                       : make_float2(0.f, 0.f);
                        }
                        lrow += (size_t)L * 2;
                        if (ltrow) ltrow += (size_t)L * 2;
                        if (step + 2 < T) {
                            lx = lrow[0]; ly = lrow[1];
                            if constexpr (kTanAhead) {
#pragma unroll
                                for (int d = 0; d < kK; ++d)
                                    if (ltrow && d < n_act) { ltx[d] = ltrow[DHTS_GN_DIR(d) * lt_dir]; lty[d] = ltrow[DHTS_GN_DIR(d) * lt_dir + 1]; }
                            }
                        }
                    }
                }
#if DHTS_MICRO_SAMPLES == 3
                if constexpr (kGN) {
                    if (due && g_on) {
                        // one observed entry per plane: x - target in float32, every product exact in double; p's terms, then v's
                        const float rp = p - g1p, rv = v - g1v;
                        if (g1p == g1p) {
                            acc[0] += (double)rp * (double)rp;
                            int i = 2 + kK;
#pragma unroll
                            for (int a = 0; a < kK; ++a) {
                                acc[2 + a] += (double)tp[a] * (double)rp;
#pragma unroll
                                for (int b = a; b < kK; ++b) acc[i++] += (double)tp[a] * (double)tp[b];
                            }
                        }
                        if (g1v == g1v) {
                            acc[1] += (double)rv * (double)rv;
                            int i = 2 + kK;
#pragma unroll
                            for (int a = 0; a < kK; ++a) {
                                acc[2 + a] += (double)tv[a] * (double)rv;
#pragma unroll
                                for (int b = a; b < kK; ++b) acc[i++] += (double)tv[a] * (double)tv[b];
                            }
                        }
                        g1p = g2p; g1v = g2v;
                        ++rj;
                        tg += g_row;
                        if (rj + 1 < g_rows) { g2p = tg[0]; g2v = tg[pr.n]; }
                    }
                } else
#endif
                if constexpr (kSamp) { if (due && col >= 0 && samples) { samples[so] = p; samples[so + pr.n] = v; } }
                else if (hist) { float *hp = hist + ((size_t)step * L + lane) * 2 * V + k; hp[0] = p; hp[V] = v; }
            }
            if constexpr (kSamp && !kGN) {
                if (due) {
                    if (col >= 0) {                      // (col >= 0 is a slot below V) slots at or beyond count: 0, as in t_hist
                        float *hp = t_samples + so;
#pragma unroll
                        for (int d = 0; d < kK; ++d)
                            if (d < n_act) { hp[d * s_dir] = tp[d]; hp[d * s_dir + pr.n] = tv[d]; }
                    }
                    so += (size_t)L * 2 * pr.n;
                }
            } else if (t_hist && k < V) {                // slots at or beyond count: 0 (their tangents never left it)
                float *hp = t_hist + ((size_t)step * L + lane) * 2 * V + k;
#pragma unroll
                for (int d = 0; d < kK; ++d)
                    if (d < n_act) { hp[d * h_dir] = tp[d]; hp[d * h_dir + V] = tv[d]; }
            }
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");     // LDS-only: hist / t_hist / samples stores stay in flight
        }
    }
    if (k < V) {
        if (!kGN || p_out != nullptr) { p_out[base + k] = p; v_out[base + k] = v; }
#pragma unroll
        for (int d = 0; d < kK; ++d)
            if (d < n_act) { t_p_out[DHTS_GN_DIR(d) * plane + base + k] = tp[d]; t_v_out[DHTS_GN_DIR(d) * plane + base + k] = tv[d]; }
    }
    if (fault_step >= 0) raise_fault(err, DHTS_FAULT_COLLISION, fault_step, lane, k);
#if DHTS_MICRO_SAMPLES == 3
    if constexpr (kGN) {
        // The lane's sums: per accumulator the target forms' pairwise tree over the slots in a fixed order (no atomics: the same bits
        // every run), kChunk accumulators a round, one plane of V doubles each -- every access of the step loop lies before a barrier
        // all threads have passed, and kChunk V doubles fit the (2 + 2 kK) (V + 1) float2 it used.  Thread 0 stores each total where
        // it belongs: sse, this launch's rows of jtr, its pairs of jtj and their mirror images.
        constexpr int kChunk = 2 + 2 * kK;
        double *A = reinterpret_cast<double *>(lds);
        int w0 = 512;
        while (w0 >= V) w0 >>= 1;                        // the largest power of two below V (0 for V = 1)
        const size_t row = (size_t)lane * gn.n_dir;
#pragma unroll
        for (int c0 = 0; c0 < kAcc; c0 += kChunk) {
            __syncthreads();
            if (k < V) {
#pragma unroll
                for (int c = 0; c < kChunk; ++c)
                    if (c0 + c < kAcc) A[(size_t)c * V + k] = acc[c0 + c];      // (a slot at or beyond count, or no probe: 0)
            }
            __syncthreads();
            for (int w = w0; w > 0; w >>= 1) {
                if (k < w && k + w < V) {
#pragma unroll
                    for (int c = 0; c < kChunk; ++c)
                        if (c0 + c < kAcc) A[(size_t)c * V + k] += A[(size_t)c * V + k + w];
                }
                __syncthreads();
            }
            if (k == 0) {
#pragma unroll
                for (int c = 0; c < kChunk; ++c) {
                    const int i = c0 + c;
                    if (i >= kAcc) continue;
                    const double x = A[(size_t)c * V];
                    if (i < 2) { if (gn.sse) gn.sse[(size_t)lane * 2 + i] = x; }
                    else if (i < 2 + kK) { if (i - 2 < n_act) gn.jtr[row + DHTS_GN_DIR(i - 2)] = x; }
                    else {
                        int j = 2 + kK;
#pragma unroll
                        for (int a = 0; a < kK; ++a)
#pragma unroll
                            for (int b = a; b < kK; ++b, ++j)
                                if (j == i && b < n_act) {
                                    gn.jtj[(row + DHTS_GN_DIR(a)) * gn.n_dir + DHTS_GN_DIR(b)] = x;
                                    gn.jtj[(row + DHTS_GN_DIR(b)) * gn.n_dir + DHTS_GN_DIR(a)] = x;
                                }
                    }
                }
            }
        }
    }
#endif
    // the lane's EARLIEST non-finite tangent, as micro_rollout_jvp_kernel records it: the minimum of (step, vehicle) through one LDS word
    if (err_jvp != nullptr) {
        unsigned *word = reinterpret_cast<unsigned *>(lds);
        __syncthreads();
        if (k == 0) *word = 0xffffffffu;
        __syncthreads();
        static_assert(DHTS_MICRO_MAX_VEHICLES <= 1024, "the vehicle takes 10 bits of the key");
        if (bad_step >= 0) atomicMin(word, ((unsigned)(bad_step < (1 << 21) - 1 ? bad_step : (1 << 21) - 1) << 10) | (unsigned)k);
        __syncthreads();
        const unsigned first = *word;
        if (k == 0 && first != 0xffffffffu) raise_fault(err_jvp, DHTS_FAULT_NAN, (int)(first >> 10), lane, (int)(first & 1023u));
    }
}
