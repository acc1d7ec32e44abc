// micro_ckpt.inc -- reverse mode of the IDM rollout without a tape in memory: the forward keeps the state every S steps, the reverse
// sweep rebuilds S steps of tape in LDS from a checkpoint, sweeps them out of LDS and moves to the checkpoint before; included by
// micro_kernels.hip inside namespace dhts, after micro_fwd_jvp.inc.
//
// What grows with T is the checkpoint buffer alone, float2 [C][L][Vp] (C = ceil(T / S), Vp = V rounded up to 64; row c = the (p, v)
// every slot of the lane enters step c S with): 8 B per vehicle per S steps against the 12 B (20 B with the parameter tape) per
// vehicle-step of micro_rollout_fwd_kernel + micro_rollout_bwd_kernel.
//
// Arithmetic: the taped pair's own.  A step forms (dp, dv) by the forward kernel's two expressions from the float32 state and calls
// idm_step, as micro_rollout_fwd_jvp_kernel does, so pT, vT, hist and the rebuilt entries (e2, e3, l3) are the forward's bits (the build
// has -ffp-contract=off and idm_step is the one place the step is written); the sweep is micro_rollout_bwd_kernel's
// one-vehicle-per-thread branch expression for expression -- dot2 with (1, dt, e2, e3) / (0, 0, -e2, l3), the g_hist add, the head's
// fold in double, the clip test e2 == e3 == l3 == 0, idm_param_jac and the sum[q] += w pj.d[q] order, the length fold, the NaN record.
//   p_in, v_in, p_out, v_out [L][V] float32      params [6][L][V] double      head [L][2] double      hist [T][L][2][V] float32 or NULL
//   g_p_in, g_v_in, g_p_out, g_v_out [L][V] float32      g_hist [T][L][2][V] float32 or NULL      g_head [L][2] double
//   g_params [6][L][V] double (kParams)

// (The dynamic LDS array of the two kernels has a name of its own, lds_ck: block-scope extern declarations of one name are one entity, and
// an aligned(16) redeclaration of `lds` after micro_rollout_bwd_kernel pads that kernel's static LDS word from 4 to 16 bytes.)

// micro_kernels.hip includes this file twice: with DHTS_MICRO_SAMPLES 0 for the two kernels described above, then with 1 for their
// sampled forms (kSamp), micro_rollout_ckpt_fwd_samples_kernel / _bwd_samples_kernel, which take MicroProbes and a samples array
// [T / every][L][2][n] in place of hist / g_hist -- siblings from one text, and the first two compile to the code they were before
// the siblings existed (profiles/micro_samples_resources*.txt).
//
// kLead, a template parameter of the two SAMPLED forms only (dhts_micro_rollout_fwd_ckpt_lead / _bwd_ckpt_lead): the head vehicle
// follows a recorded leader, MicroLead's lead [T][L][2] float32 = the (p, v) it is seen at in step t, as every other vehicle follows
// the slot in front of it -- the same two expressions for (dp, dv), the same idm_step; half_len with lead_length (or the head's own
// length); no head gap is read and no g_head written.  The head's thread owns the leader's slot n of S (and of X): it writes row
// t + 1 there during step t, the row after that in flight in registers; the reverse sweep stores C1[n], the cotangent of the slot in
// front of the head, as row t of g_lead [T][L][2] instead of folding it into the head.  A NULL samples / g_samples: nothing is observed.
// kLead = false is the code the sampled forms were before (profiles/micro_lead_resources*.txt).
//
// The boundary is three-valued: the template parameter of the sampled and the target forms is MicroBoundary kB (micro_kernels.hip), and
// kHeadGap / kLead / kRing below name its values.  kRing (dhts_micro_rollout_fwd_ckpt_ring / _bwd_ckpt_ring and the _target_ring pair): a
// ring road.  The head follows the image of the lane's own tail one circumference ahead, ((float)((double)p_tail + ring[lane]), v_tail)
// of the tail's state before the step, by the followers' expressions; half_len of the head is (length[0] + length[head]) / 2.  The
// TAIL's thread (k == 0) owns slot n of S: row 0 before the first barrier, S[(q ^ 1) P + n] from its new (p, v) beside its own store in
// every step -- no global load, nothing in flight; the head's thread still records X[r][n] = ls under kParams.  The reverse sweep adds
// C1[n] to the tail's (np_, nv_) in the same sweep step (the float cast has derivative 1) and nothing to the head; no g_head, no g_lead;
// g_params[5][0] = -0.5 (A[0] + A[n - 1]).  ring is read once per lane.  kB = kBoundHead / kBoundLead are the code the forms were before
// (profiles/micro_ring_resources*.txt).
//
// A third pass, DHTS_MICRO_SAMPLES 2, gives the TARGET forms (kTarget; dhts_micro_rollout_fwd_ckpt_target / _bwd_ckpt_target),
// micro_rollout_ckpt_fwd_target_kernel<kLead> / _bwd_target_kernel<kParams, kLead>: the trajectory-fit loss inside the pair.  They
// take target [T][L][2][V] float32 (hist's indexing: the observed (p, v) after step t; NaN = not observed) where the first pair takes
// hist / g_hist, and neither array exists.  The forward sums, per thread and in step order, the squares (in double) of the float32
// residuals x - target into two doubles, reduces them over the workgroup in a fixed order through the LDS the step loop is done with
// and writes sse [L][2] double; the reverse replay forms the finished cotangent pair (float)(2 g_sse[l][c]) * (x - target) from the
// post-step state it has just recomputed and keeps it in two more planes of R, from where the sweep adds it where g_hist is added.
// Rows of target travel in registers ahead of the step that uses them, as the lead rows do.  kTarget = false (passes 0 and 1) is the
// code the kernels were before (profiles/micro_target_resources*.txt).

#if DHTS_MICRO_SAMPLES == 0
// dynamic LDS of the two kernels: the plan (micro_plan) and the kernels' own carving read these
__host__ __device__ inline size_t micro_ckpt_fwd_lds_bytes(int V) { return sizeof(float2) * 2 * (size_t)(V + 1); }
// reverse, fixed part: the replay's state hand-over S[2][V + 1] and the four cotangent arrays of V + 2 floats
__host__ __device__ inline size_t micro_ckpt_bwd_fixed_bytes(int V) { return sizeof(float2) * 2 * (size_t)(V + 1) + sizeof(float) * 4 * (size_t)(V + 2); }
// ... and per step of the segment ring: the entry (e2, e3, l3) per vehicle, with kParams also the pre-step (p, v) over V + 1 slots,
// in the target forms two more planes of R, the finished cotangent pair of the step (their forward reduces in S: 16 V <= 16 (V + 1))
__host__ __device__ inline size_t micro_ckpt_bwd_step_bytes(int V, bool params, bool target) {
    return sizeof(MicroTape3) * (size_t)V + (params ? sizeof(float2) * (size_t)(V + 1) : 0) + (target ? sizeof(float) * 2 * (size_t)V : 0);
}
__host__ __device__ inline size_t micro_ckpt_bwd_lds_bytes(int V, int S, bool params, bool target) {
    return micro_ckpt_bwd_fixed_bytes(V) + (size_t)S * micro_ckpt_bwd_step_bytes(V, params, target);
}
// one observed entry pair of the forward: hist - observed in float32, squared and summed in double; a NaN entry is not observed
__device__ inline void micro_target_add(float p, float v, float tp, float tv, double &ap, double &av) {
    const float rp = p - tp, rv = v - tv;
    if (tp == tp) ap += (double)rp * (double)rp;
    if (tv == tv) av += (double)rv * (double)rv;
}
#endif

// grid = L workgroups (one traffic lane each) of blockDim.x >= V threads (V rounded up to 64): micro_rollout_fwd_jvp_kernel's mapping
// without tangents -- one vehicle per thread, its float32 (p, v) and derived parameters in registers for all T steps, the new state left
// in S [copy][slot] for the follower, copies alternating with the step parity: ONE barrier per step, and that one waits for LDS only
// (checkpoint and hist stores stay in flight across it).  Dynamic LDS: float2 S[2][V + 1].
// Before step c Sg every slot of the lane (live or not) stores its (p, v) to row c of ckpt.
// err: DHTS_FAULT_COLLISION where idm_step reported one, as the forward kernel reports it.  A block smaller than the lane:
// DHTS_FAULT_CAPACITY (index -3), outputs NaN (the launch sizes the block from the same plan: it does not happen).
// kSamp (micro_rollout_ckpt_fwd_samples_kernel): instead of hist, row j of samples [T / every][L][2][n] takes (p, v) of the probe
// slots after step (j + 1) every - 1 -- a thread finds its slot's column among the probes once, before the step loop, counts the steps
// down to the next sampled one and moves a running pointer from row to row; a slot at or beyond count stores nothing.  ckpt may then
// be NULL: no checkpoint is kept (a forward that nobody differentiates).
// kTarget (micro_rollout_ckpt_fwd_target_kernel): no hist and no samples; the thread of a live slot holds the next two rows of its
// column of target in (tp1, tv1), (tp2, tv2) and adds the squared residuals of observed entries to (ap, av); sse [L][2] is written by
// thread 0 after the block reduction (NaN where the block is smaller than the lane).  ckpt may be NULL as with kSamp.
#if DHTS_MICRO_SAMPLES == 0
__global__ __launch_bounds__(1024) void micro_rollout_ckpt_fwd_kernel(
    int L, int V, int T, int Sg, double dt, const float *__restrict__ p_in, const float *__restrict__ v_in,
    const int32_t *__restrict__ count, const double *__restrict__ params, const double *__restrict__ head,
    float *__restrict__ p_out, float *__restrict__ v_out, float2 *__restrict__ ckpt, float *__restrict__ hist, dhts_error *err) {
    constexpr bool kSamp = false, kLead = false, kRing = false, kHeadGap = true, kTarget = false;
    const MicroProbes pr = {};
    float *const samples = nullptr;
    const MicroLead ld = {};
    const float *const target = nullptr;
    double *const sse = nullptr;
#elif DHTS_MICRO_SAMPLES == 2
template <MicroBoundary kB>
__global__ __launch_bounds__(1024) void micro_rollout_ckpt_fwd_target_kernel(
    int L, int V, int T, int Sg, double dt, const float *__restrict__ p_in, const float *__restrict__ v_in,
    const int32_t *__restrict__ count, const double *__restrict__ params, const double *__restrict__ head,
    float *__restrict__ p_out, float *__restrict__ v_out, float2 *__restrict__ ckpt, const float *__restrict__ target,
    double *__restrict__ sse, dhts_error *err, MicroLead ld) {
    constexpr bool kSamp = false, kTarget = true, kLead = kB == kBoundLead, kRing = kB == kBoundRing, kHeadGap = kB == kBoundHead;
    const MicroProbes pr = {};
    float *const samples = nullptr;
    float *const hist = nullptr;
#else
template <MicroBoundary kB>
__global__ __launch_bounds__(1024) void micro_rollout_ckpt_fwd_samples_kernel(
    int L, int V, int T, int Sg, double dt, const float *__restrict__ p_in, const float *__restrict__ v_in,
    const int32_t *__restrict__ count, const double *__restrict__ params, const double *__restrict__ head,
    float *__restrict__ p_out, float *__restrict__ v_out, float2 *__restrict__ ckpt, MicroProbes pr, float *__restrict__ samples,
    dhts_error *err, MicroLead ld) {
    constexpr bool kSamp = true, kTarget = false, kLead = kB == kBoundLead, kRing = kB == kBoundRing, kHeadGap = kB == kBoundHead;
    float *const hist = nullptr;
    const float *const target = nullptr;
    double *const sse = nullptr;
#endif
    extern __shared__ __attribute__((aligned(16))) float lds_ck[];
    const int lane = blockIdx.x;
    const int k = threadIdx.x;
    const int B = blockDim.x;
    const int P = V + 1;
    float2 *S = reinterpret_cast<float2 *>(lds_ck);         // [copy][P]
    const size_t base = (size_t)lane * V;
    const size_t plane = (size_t)L * V;
    const int Vp = (V + 63) & ~63;
    const int nc = count ? count[lane] : V;
    const int n = nc < 0 ? 0 : (nc > V ? V : nc);       // (no slot outside the lane is ever addressed)
    const bool vk = k < n;
    const bool is_head = k == n - 1;
    const int kc = k < V ? k : 0;
    const double inv_dt = 1.0 / dt;

    if (V > B) {
        const float nanf_ = __builtin_nanf("");
        for (int i = k; i < V; i += B) { p_out[base + i] = nanf_; v_out[base + i] = nanf_; }
        if constexpr (kSamp) { if (kHeadGap || samples) micro_samples_fill(samples, pr, T, L, lane, k, B, nanf_); }
        if constexpr (kTarget) { if (k == 0) { sse[(size_t)lane * 2] = (double)nanf_; sse[(size_t)lane * 2 + 1] = (double)nanf_; } }
        if (k == 0) raise_fault(err, DHTS_FAULT_CAPACITY, 0, lane, -3);
        return;
    }

    float p = p_in[base + kc], v = v_in[base + kc];      // (a slot at or beyond count keeps them: the outputs pass it through)
    const int col = kSamp ? ((!kHeadGap && samples == nullptr) ? -1 : micro_probe_column(pr, k, V)) : -1;     // kLead, kRing, no samples: no column
    IdmDerived prm = {};
    double half_len = 0.;
    if (vk) {
        IdmParams raw;
        raw.a_max = params[0 * plane + base + k]; raw.a_pref = params[1 * plane + base + k];
        raw.v_target = params[2 * plane + base + k]; raw.min_space = params[3 * plane + base + k];
        raw.time_pref = params[4 * plane + base + k]; raw.length = params[5 * plane + base + k];
        prm = idm_derive(raw);
        idm_set_dt(prm, dt);
        const int kl = k + 1 < n ? k + 1 : (kRing ? 0 : k);      // kRing: the head's leader is the tail
        half_len = (params[5 * plane + base + kl] + raw.length) * 0.5;
        if constexpr (kLead) { if (is_head && ld.length) half_len = (ld.length[lane] + raw.length) * 0.5; }
    }
    double head_dp = 0., head_dv = 0., ring = 0.;
    if constexpr (kRing) ring = ld.ring[lane];
    else if constexpr (!kLead) { head_dp = head[(size_t)lane * 2]; head_dv = head[(size_t)lane * 2 + 1]; }

    for (int i = k; i < 2 * P; i += B) S[i] = make_float2(0.f, 0.f);
    __syncthreads();

    int fault_step = -1;
    double ap = 0., av = 0.;           // kTarget: this vehicle's squared residuals, summed in step order
    if (T > 0) {
        if (vk) S[k] = make_float2(p, v);
        // kRing: the TAIL's thread owns slot n of S -- its own state one circumference ahead, beside every store of its own
        if constexpr (kRing) { if (vk && k == 0) S[n] = make_float2((float)((double)p + ring), v); }
        // kLead: the head's thread owns slot n of S -- row 0 now, row step + 1 during step `step`, the row after that in flight in (lx, ly)
        const float *lrow = nullptr;
        float lx = 0.f, ly = 0.f;
        if constexpr (kLead) {
            if (is_head) {
                lrow = micro_lead_row(ld.lead, lane);
                S[n] = make_float2(lrow[0], lrow[1]);
                lrow += (size_t)L * 2;
                if (T > 1) { lx = lrow[0]; ly = lrow[1]; }
            }
        }
        __syncthreads();
        float2 *ck = ckpt + (size_t)lane * Vp + k;       // this slot of row 0; a row is L Vp entries
        int next_ck = ((kSamp || kTarget) && ckpt == nullptr) ? -1 : 0;
        float *sp = nullptr;                             // kSamp: this slot's column of the next row; a row is L 2 n floats
        int cd = 0;                                      // ... and the steps until that row is due
        if constexpr (kSamp) { sp = samples + (size_t)lane * 2 * pr.n + (col < 0 ? 0 : col); cd = pr.every; }
        // kTarget: this slot's column of the row to load next (a row is L 2 V floats); rows step and step + 1 are in the registers
        const float *tg = nullptr;
        float tp1 = 0.f, tv1 = 0.f, tp2 = 0.f, tv2 = 0.f;
        if constexpr (kTarget) {
            // (p, v) arrive here, before the first row of target is asked for: left pending across the loop's entry, their loads would
            // make every step wait for every load issued since (the wait counter is one for all of them, in order)
            asm volatile("" : "+v"(p), "+v"(v));
            if (vk) {
                tg = target + (size_t)lane * 2 * V + k;
                tp1 = tg[0]; tv1 = tg[V];
                tg += (size_t)L * 2 * V;
                if (T > 1) { tp2 = tg[0]; tv2 = tg[V]; }
            }
        }
        for (int step = 0; step < T; ++step) {
            const int q = step & 1;
            bool due = false;
            if constexpr (kSamp) { due = --cd == 0; cd = due ? pr.every : cd; }
            if (step == next_ck) {
                if (k < V) *ck = make_float2(p, v);
                ck += (size_t)L * Vp;
                next_ck += Sg;
            }
            if (vk) {
                const float2 ls = S[q * P + k + 1];      // the leader's state before this step
                const double pd = p, vd = v;
                // compute_state_delta, _micro_lane.py:201-212, in the forward kernel's expressions
                const double dp = (kHeadGap && is_head) ? head_dp : fabs((double)ls.x - pd) - half_len;
                const double dv = (kHeadGap && is_head) ? head_dv : vd - (double)ls.y;
                IdmStep o;
                idm_step(pd, vd, dp, dv, prm, dt, inv_dt, o);
                if (o.collided && fault_step < 0) fault_step = step;
                p = o.np; v = o.nv;
                S[(q ^ 1) * P + k] = make_float2(p, v);      // what this vehicle enters step + 1 with
                if constexpr (kRing) { if (k == 0) S[(q ^ 1) * P + n] = make_float2((float)((double)p + ring), v); }
                if constexpr (kLead) {
                    if (is_head && step + 1 < T) {
                        S[(q ^ 1) * P + n] = make_float2(lx, ly);      // ... and what its leader is seen at in step + 1
                        lrow += (size_t)L * 2;
                        if (step + 2 < T) { lx = lrow[0]; ly = lrow[1]; }
                    }
                }
                if constexpr (kTarget) {
                    micro_target_add(p, v, tp1, tv1, ap, av);
                    tp1 = tp2; tv1 = tv2;
                    tg += (size_t)L * 2 * V;
                    if (step + 2 < T) { tp2 = tg[0]; tv2 = tg[V]; }
                }
                if constexpr (kSamp) { if (due && col >= 0) { sp[0] = p; sp[pr.n] = v; } }
                else if (hist) { float *hp = hist + ((size_t)step * L + lane) * 2 * V + k; hp[0] = p; hp[V] = v; }
            }
            if constexpr (kSamp) { if (due) sp += (size_t)L * 2 * pr.n; }
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");     // LDS-only: checkpoint, hist and samples stores stay in flight
        }
    }
    if (k < V) { p_out[base + k] = p; v_out[base + k] = v; }
    if (fault_step >= 0) raise_fault(err, DHTS_FAULT_COLLISION, fault_step, lane, k);
    if constexpr (kTarget) {
        // the lane's two sums: a pairwise tree over the slots in a fixed order (no atomics: the same bits every run), in S -- every
        // access of the step loop lies before a barrier all threads have passed, and V entries of 16 B fit its 2 (V + 1) of 8 B
        double2 *A = reinterpret_cast<double2 *>(lds_ck);
        if (k < V) A[k] = make_double2(ap, av);         // (a slot at or beyond count: 0)
        __syncthreads();
        int w = 512;
        while (w >= V) w >>= 1;                          // the largest power of two below V (0 for V = 1)
        for (; w > 0; w >>= 1) {
            if (k < w && k + w < V) { const double2 a = A[k], b = A[k + w]; A[k] = make_double2(a.x + b.x, a.y + b.y); }
            __syncthreads();
        }
        if (k == 0) { const double2 a = A[0]; sse[(size_t)lane * 2] = a.x; sse[(size_t)lane * 2 + 1] = a.y; }
    }
}

// grid = L workgroups of blockDim.x >= V threads, one vehicle per thread.  Dynamic LDS (micro_ckpt_bwd_lds_bytes):
//   float2 S[2][V + 1]             the replay's state hand-over, as in the forward
//   float2 X[Sg][V + 1]            kParams: the (p, v) a vehicle entered step r of the segment with (slot V is never written nor used;
//                                  kLead: slot n holds the leader the head saw in step r, written and read by the head's thread)
//   float  Gp, Gv, C1p, C1v [V + 2]    the cotangents, as in micro_rollout_bwd_kernel (C1[i + 1] = dLeading[i]^T g[i])
//   float  R[Sg][3][V]             the segment's tape: e2, e3, l3 of step r, one plane each
// Segments c = C - 1 .. 0: load row c of ckpt (prefetched while the segment after it was swept), replay steps [c Sg, min(T, (c + 1) Sg))
// into R (and X), one LDS-only barrier per step, then sweep them newest first.  A thread reads back only its own entries of R and X;
// the leader's X[r][k + 1] is another thread's, and the barrier that ends the replay's last step is what it waits for.  The replay
// raises no collision: the forward did.  g_hist rows travel two steps ahead in registers, as in micro_rollout_bwd_kernel.
// err: DHTS_FAULT_NAN at the latest step, lowest vehicle, where a non-finite cotangent appeared.
// kSamp (micro_rollout_ckpt_bwd_samples_kernel): g_samples [T / every][L][2][n] takes g_hist's place -- only the thread of a live probe
// slot adds, and only at a sampled step.  Its rows travel two ROWS ahead in the same four registers (2 every steps: with every = 1
// the g_hist pipeline), across segment boundaries like the countdown to the next sampled step, which starts at T mod every: the
// trailing steps have no row.
// kTarget (micro_rollout_ckpt_bwd_target_kernel): R has five planes per step -- the replay, which holds the post-step (p, v) of step r
// in registers, adds (float)(2 g_sse[lane][c]) * (x - target) (0 for a NaN entry) as planes 3 and 4, and the sweep adds them where
// g_hist is added: no global load in the sweep.  The target row of a segment's first step travels like ck, a segment ahead in
// (t0p, t0v); the rows of its later steps one replay step ahead in (t1p, t1v) -- the lead rows' pipeline, on every live thread.
#if DHTS_MICRO_SAMPLES == 0
template <bool kParams>
__global__ __launch_bounds__(1024) void micro_rollout_ckpt_bwd_kernel(
    int L, int V, int T, int Sg, double dt, const float2 *__restrict__ ckpt, const int32_t *__restrict__ count,
    const double *__restrict__ params, const double *__restrict__ head, const float *__restrict__ g_p_in,
    const float *__restrict__ g_v_in, const float *__restrict__ g_hist, float *__restrict__ g_p_out, float *__restrict__ g_v_out,
    double *__restrict__ g_head, double *__restrict__ g_params, dhts_error *err) {
    constexpr bool kSamp = false, kLead = false, kRing = false, kHeadGap = true, kTarget = false;
    const MicroProbes pr = {};
    const float *const g_samples = nullptr;
    const MicroLead ld = {};
    const float *const target = nullptr;
    const double *const g_sse = nullptr;
#elif DHTS_MICRO_SAMPLES == 2
template <bool kParams, MicroBoundary kB>
__global__ __launch_bounds__(1024) void micro_rollout_ckpt_bwd_target_kernel(
    int L, int V, int T, int Sg, double dt, const float2 *__restrict__ ckpt, const int32_t *__restrict__ count,
    const double *__restrict__ params, const double *__restrict__ head, const float *__restrict__ g_p_in,
    const float *__restrict__ g_v_in, const float *__restrict__ target, const double *__restrict__ g_sse, float *__restrict__ g_p_out,
    float *__restrict__ g_v_out, double *__restrict__ g_head, double *__restrict__ g_params, dhts_error *err, MicroLead ld) {
    constexpr bool kSamp = false, kTarget = true, kLead = kB == kBoundLead, kRing = kB == kBoundRing, kHeadGap = kB == kBoundHead;
    const MicroProbes pr = {};
    const float *const g_samples = nullptr;
    const float *const g_hist = nullptr;
#else
template <bool kParams, MicroBoundary kB>
__global__ __launch_bounds__(1024) void micro_rollout_ckpt_bwd_samples_kernel(
    int L, int V, int T, int Sg, double dt, const float2 *__restrict__ ckpt, const int32_t *__restrict__ count,
    const double *__restrict__ params, const double *__restrict__ head, const float *__restrict__ g_p_in,
    const float *__restrict__ g_v_in, MicroProbes pr, const float *__restrict__ g_samples, float *__restrict__ g_p_out,
    float *__restrict__ g_v_out, double *__restrict__ g_head, double *__restrict__ g_params, dhts_error *err, MicroLead ld) {
    constexpr bool kSamp = true, kTarget = false, kLead = kB == kBoundLead, kRing = kB == kBoundRing, kHeadGap = kB == kBoundHead;
    const float *const g_hist = nullptr;
    const float *const target = nullptr;
    const double *const g_sse = nullptr;
#endif
    extern __shared__ __attribute__((aligned(16))) float lds_ck[];
    const int lane = blockIdx.x;
    const int k = threadIdx.x;
    const int B = blockDim.x;
    const int P1 = V + 1, P = V + 2;
    float2 *S = reinterpret_cast<float2 *>(lds_ck);
    float2 *X = S + 2 * P1;
    float *Gp = reinterpret_cast<float *>(X + (kParams ? (size_t)Sg * P1 : 0));
    float *Gv = Gp + P, *C1p = Gp + 2 * P, *C1v = Gp + 3 * P;
    float *R = Gp + 4 * P;
    constexpr int kPlanes = kTarget ? 5 : 3;            // of R per step
    const size_t base = (size_t)lane * V;
    const size_t plane = (size_t)L * V;
    const int Vp = (V + 63) & ~63;
    const int nc = count ? count[lane] : V;
    const int n = nc < 0 ? 0 : (nc > V ? V : nc);
    const bool vk = k < n;
    const bool is_head = k == n - 1;
    const int kc = k < V ? k : 0;
    const double inv_dt = 1.0 / dt;
    const float dtf = (float)dt;

    if (V > B) {
        const float nanf_ = __builtin_nanf("");
        for (int i = k; i < V; i += B) { g_p_out[base + i] = nanf_; g_v_out[base + i] = nanf_; }
        if constexpr (kLead) micro_lead_fill(ld.g_lead, T, L, lane, k, B, nanf_);
        if (k == 0) raise_fault(err, DHTS_FAULT_CAPACITY, 0, lane, -3);
        return;
    }
    if constexpr (kLead) { if (n == 0) micro_lead_fill(ld.g_lead, T, L, lane, k, B, 0.f); }      // (no head: nobody else writes the rows)

    for (int i = k; i < P; i += B) { Gp[i] = 0.f; Gv[i] = 0.f; C1p[i] = 0.f; C1v[i] = 0.f; }
    for (int i = k; i < 2 * P1; i += B) S[i] = make_float2(0.f, 0.f);
    __syncthreads();
    if (vk) { Gp[k] = g_p_in[base + k]; Gv[k] = g_v_in[base + k]; }

    // this thread's vehicle: the forward's derived parameters for the replay, the reverse sweep's for the partials
    IdmDerived prm = {};
    IdmParamDerived pm = {};
    double half_len = 0.;
    double sum[6] = {0., 0., 0., 0., 0., 0.};           // a_max, a_pref, v_target, min_space, time_pref, gap
    if (vk) {
        IdmParams raw;
        raw.a_max = params[0 * plane + base + k]; raw.a_pref = params[1 * plane + base + k];
        raw.v_target = params[2 * plane + base + k]; raw.min_space = params[3 * plane + base + k];
        raw.time_pref = params[4 * plane + base + k]; raw.length = params[5 * plane + base + k];
        prm = idm_derive(raw);
        idm_set_dt(prm, dt);
        if constexpr (kParams) pm = idm_param_derive(raw);
        half_len = (params[5 * plane + base + (k + 1 < n ? k + 1 : (kRing ? 0 : k))] + raw.length) * 0.5;
        if constexpr (kLead) { if (is_head && ld.length) half_len = (ld.length[lane] + raw.length) * 0.5; }
    }
    double head_dp = 0., head_dv = 0., ring = 0.;
    if constexpr (kRing) ring = ld.ring[lane];
    else if constexpr (!kLead) { head_dp = head[(size_t)lane * 2]; head_dv = head[(size_t)lane * 2 + 1]; }
    __syncthreads();

    double gh_p = 0., gh_v = 0.;       // held by the thread that owns the head vehicle
    int bad_step = -1;                 // first non-finite cotangent this thread meets (the latest step: the sweep runs backwards)
    const int C = T > 0 ? (T + Sg - 1) / Sg : 0;
    if (C > 0) {
        const size_t row = (size_t)L * Vp;
        const float2 *ck0 = ckpt + (size_t)lane * Vp + kc;
        float2 ck = ck0[(size_t)(C - 1) * row];
        const float *gh0 = g_hist ? g_hist + (size_t)lane * 2 * V + kc : nullptr;
        const size_t h_stride = (size_t)L * 2 * V;
        float hp1 = 0.f, hv1 = 0.f, hp2 = 0.f, hv2 = 0.f;
        if (gh0) {
            const float *a = gh0 + (size_t)(T - 1) * h_stride, *b = gh0 + (size_t)(T > 1 ? T - 2 : 0) * h_stride;
            hp1 = a[0]; hv1 = a[V]; hp2 = b[0]; hv2 = b[V];
        }
        // kSamp: does this thread add at a sampled step; its column of the row to load next (rows_left of them are still unloaded);
        // steps to sweep before the next sampled one
        bool probe = false;
        const float *gs = nullptr;
        int rows_left = 0, cd = 0;
        const size_t s_row = kSamp ? (size_t)L * 2 * pr.n : 0;
        if constexpr (kSamp) {
            const int col = micro_probe_column(pr, k, V);
            const int rows = T / pr.every;
            probe = vk && col >= 0 && (kHeadGap || g_samples != nullptr);      // kLead, kRing, no g_samples: nothing was observed
            cd = T - rows * pr.every;
            if (probe && rows > 0) {
                gs = g_samples + (size_t)(rows - 1) * s_row + (size_t)lane * 2 * pr.n + col;
                hp1 = gs[0]; hv1 = gs[pr.n];
                rows_left = rows - 1;
                if (rows_left > 0) { gs -= s_row; hp2 = gs[0]; hv2 = gs[pr.n]; --rows_left; }
            }
        }
        // kLead: the head's thread owns slot n of S (and of X): the lead row of a segment's first step travels like ck, a segment
        // ahead in (l0x, l0y); the rows of its later steps one replay step ahead in (l1x, l1y)
        // kTarget: this slot's column of row 0 of target; twice the cotangent of the lane's two sums, in float32
        const float *const tg0 = (kTarget && vk) ? target + (size_t)lane * 2 * V + k : nullptr;
        float t0p = 0.f, t0v = 0.f, t1p = 0.f, t1v = 0.f, g2p = 0.f, g2v = 0.f;
        if constexpr (kTarget) {
            if (g_sse) { g2p = (float)(2. * g_sse[(size_t)lane * 2]); g2v = (float)(2. * g_sse[(size_t)lane * 2 + 1]); }
            if (vk) { const float *a = tg0 + (size_t)(C - 1) * Sg * h_stride; t0p = a[0]; t0v = a[V]; }
        }
        const float *const lead0 = (kLead && is_head) ? micro_lead_row(ld.lead, lane) : nullptr;
        const size_t l_row = (size_t)L * 2;
        float l0x = 0.f, l0y = 0.f, l1x = 0.f, l1y = 0.f;
        if constexpr (kLead) {
            if (is_head) { const float *a = lead0 + (size_t)(C - 1) * Sg * l_row; l0x = a[0]; l0y = a[1]; }
        }
        for (int c = C - 1; c >= 0; --c) {
            const int s0 = c * Sg, s1 = (T - s0 < Sg) ? T : s0 + Sg;
            float p = ck.x, v = ck.y;
            ck = ck0[(size_t)(c > 0 ? c - 1 : 0) * row];         // the checkpoint before: in flight across the whole segment
            // ---- replay steps [s0, s1) into the ring ----
            if (vk) S[k] = make_float2(p, v);
            if constexpr (kRing) { if (vk && k == 0) S[n] = make_float2((float)((double)p + ring), v); }      // the tail, one circumference ahead
            if constexpr (kLead) {
                if (is_head) {
                    S[n] = make_float2(l0x, l0y);
                    if (s0 + 1 < s1) { const float *a = lead0 + (size_t)(s0 + 1) * l_row; l1x = a[0]; l1y = a[1]; }
                    const float *b = lead0 + (size_t)(c > 0 ? s0 - Sg : 0) * l_row;
                    l0x = b[0]; l0y = b[1];
                }
            }
            float tcp = 0.f, tcv = 0.f;                          // kTarget: the target row of the step the replay is at
            if constexpr (kTarget) {
                if (vk) {
                    tcp = t0p; tcv = t0v;
                    if (s0 + 1 < s1) { const float *a = tg0 + (size_t)(s0 + 1) * h_stride; t1p = a[0]; t1v = a[V]; }
                    const float *b = tg0 + (size_t)(c > 0 ? s0 - Sg : 0) * h_stride;
                    t0p = b[0]; t0v = b[V];
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            for (int r = 0; r < s1 - s0; ++r) {
                const int q = r & 1;
                if (vk) {
                    const float2 ls = S[q * P1 + k + 1];
                    const double pd = p, vd = v;
                    // compute_state_delta, _micro_lane.py:201-212, in the forward kernel's expressions
                    const double dp = (kHeadGap && is_head) ? head_dp : fabs((double)ls.x - pd) - half_len;
                    const double dv = (kHeadGap && is_head) ? head_dv : vd - (double)ls.y;
                    IdmStep o;
                    idm_step(pd, vd, dp, dv, prm, dt, inv_dt, o);
                    float *e = R + (size_t)r * kPlanes * V + k;
                    e[0] = o.dE[2]; e[V] = o.dE[3]; e[2 * V] = o.dLd[3];
                    if constexpr (kParams) X[(size_t)r * P1 + k] = make_float2(p, v);
                    p = o.np; v = o.nv;
                    S[(q ^ 1) * P1 + k] = make_float2(p, v);
                    if constexpr (kRing) {
                        if (k == 0) S[(q ^ 1) * P1 + n] = make_float2((float)((double)p + ring), v);
                        if constexpr (kParams) { if (is_head) X[(size_t)r * P1 + n] = ls; }      // the image the head saw in this step
                    }
                    if constexpr (kTarget) {
                        // the finished cotangent pair of this step: 2 g (hist - observed), the forward's float32 residual
                        e[3 * V] = (tcp == tcp) ? g2p * (p - tcp) : 0.f;
                        e[4 * V] = (tcv == tcv) ? g2v * (v - tcv) : 0.f;
                        if (s0 + r + 1 < s1) {
                            tcp = t1p; tcv = t1v;
                            if (s0 + r + 2 < s1) { const float *a = tg0 + (size_t)(s0 + r + 2) * h_stride; t1p = a[0]; t1v = a[V]; }
                        }
                    }
                    if constexpr (kLead) {
                        if (is_head) {
                            if constexpr (kParams) X[(size_t)r * P1 + n] = ls;      // the leader the head saw in this step
                            if (s0 + r + 1 < s1) {
                                S[(q ^ 1) * P1 + n] = make_float2(l1x, l1y);
                                if (s0 + r + 2 < s1) { const float *a = lead0 + (size_t)(s0 + r + 2) * l_row; l1x = a[0]; l1y = a[1]; }
                            }
                        }
                    }
                }
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            }
            // ---- sweep them newest first, out of the ring ----
            for (int step = s1 - 1; step >= s0; --step) {
                const int r = step - s0;
                const float chp = hp1, chv = hv1;
                bool due = false;
                if constexpr (kSamp) {
                    due = cd == 0;
                    cd = due ? pr.every - 1 : cd - 1;
                    if (due) {
                        hp1 = hp2; hv1 = hv2;
                        if (rows_left > 0) { gs -= s_row; hp2 = gs[0]; hv2 = gs[pr.n]; --rows_left; }      // (rows_left > 0 on a probe's thread only)
                    }
                } else {
                    hp1 = hp2; hv1 = hv2;
                    if (gh0) { const float *a = gh0 + (size_t)(step > 1 ? step - 2 : 0) * h_stride; hp2 = a[0]; hv2 = a[V]; }
                }
                MicroTape3 e = {0.f, 0.f, 0.f};
                float2 cx = make_float2(0.f, 0.f);
                float gv_step = 0.f;
                if (vk) {
                    const float *er = R + (size_t)r * kPlanes * V + k;
                    e.e2 = er[0]; e.e3 = er[V]; e.l3 = er[2 * V];
                    float gp = Gp[k], gv = Gv[k];
                    if constexpr (kTarget) { gp += er[3 * V]; gv += er[4 * V]; }
                    else if constexpr (kSamp) { if (due && probe) { gp += chp; gv += chv; } }
                    else if (gh0) { gp += chp; gv += chv; }
                    Gp[k] = dot2(1.f, gp, e.e2, gv);           // grad_ps[:-1] = dqs[:, 0]^T g
                    Gv[k] = dot2(dtf, gp, e.e3, gv);
                    C1p[k + 1] = dot2(0.f, gp, -e.e2, gv);     // grad_ps[1:] += dqs[:, 1]^T g
                    C1v[k + 1] = dot2(0.f, gp, e.l3, gv);
                    if constexpr (kParams) { cx = X[(size_t)r * P1 + k]; gv_step = gv; }
                }
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
                if constexpr (kParams) {
                    if (vk) {
                        // compute_state_delta and the collision / clamp rules of the forward, _micro_lane.py:149-166, 201-212
                        const float2 xl = X[(size_t)r * P1 + k + 1];
                        const double pv = cx.y;
                        double gap = (kHeadGap && is_head) ? head_dp : fabs((double)xl.x - (double)cx.x) - half_len;
                        double dv = (kHeadGap && is_head) ? head_dv : pv - (double)xl.y;
                        const bool live_gap = (!kHeadGap || !is_head) && gap >= 1e-5;       // else a constant: nothing flows to the lengths
                        if (gap < 0) { gap = 0; dv = 0; }
                        gap = (1e-5 > gap) ? 1e-5 : gap;
                        if (!(e.e2 == 0.f && e.e3 == 0.f && e.l3 == 0.f)) {  // (the forward's acceleration clip zeroes all three)
                            IdmParamJac pj;
                            idm_param_jac(pv, gap, dv, pm, dt, pj);
                            const double w = (double)gv_step * dt;
#pragma unroll
                            for (int q = 0; q < 5; ++q) sum[q] += w * pj.d[q];
                            if (live_gap) sum[5] += w * pj.d[5];
                        }
                    }
                }
                if (vk) {
                    float np_ = Gp[k], nv_ = Gv[k];
                    if (k > 0) { np_ += C1p[k]; nv_ += C1v[k]; }
                    if constexpr (kLead) {
                        // the prescribed leader's cotangent C1[n] is this step's row of g_lead: nothing returns to the head
                        if (is_head) { float *gl = ld.g_lead + ((size_t)step * L + lane) * 2; gl[0] = C1p[n]; gl[1] = C1v[n]; }
                    } else if constexpr (kRing) {
                        // the image is the tail's own state (the float cast has derivative 1): C1[n] returns to the tail, nothing to the head
                        if (k == 0) { np_ += C1p[n]; nv_ += C1v[n]; }
                    } else if (is_head) {
                        // virtual leader = (p_head + head_dp, v_head - head_dv): its cotangent C1[n] returns to the head
                        const float vp = C1p[n], vv = C1v[n];
                        gh_p += (double)vp;
                        gh_v -= (double)vv;
                        np_ += vp; nv_ += vv;
                    }
                    Gp[k] = np_; Gv[k] = nv_;
                    if (bad_step < 0 && !(isfinite(np_) && isfinite(nv_))) bad_step = step;
                }
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            }
        }
    }
    __syncthreads();
    if (k < V) {
        g_p_out[base + k] = vk ? Gp[k] : 0.f;
        g_v_out[base + k] = vk ? Gv[k] : 0.f;
    }
    if constexpr (kParams) {
        // length enters a gap as -(len_leader + len) / 2 (_micro_lane.py:211): a vehicle's own gap sum and its follower's
        double *A = reinterpret_cast<double *>(C1p);            // (C1p, C1v: 2 P floats = P doubles; the sweeps are done with them)
        __syncthreads();
        if (k < V) A[k] = vk ? sum[5] : 0.;
        __syncthreads();
        if (k < V) {
#pragma unroll
            for (int q = 0; q < 5; ++q) g_params[q * plane + base + k] = vk ? sum[q] : 0.;
            // (kRing: the tail is the head's leader, its length is in the head's gap as well)
            g_params[5 * plane + base + k] = vk ? -0.5 * (A[k] + (k > 0 ? A[k - 1] : (kRing ? A[n - 1] : 0.))) : 0.;
        }
    }
    if (g_head) {
        if (n == 0) { if (k == 0) { g_head[(size_t)lane * 2] = 0.; g_head[(size_t)lane * 2 + 1] = 0.; } }
        else if (is_head) { g_head[(size_t)lane * 2] = gh_p; g_head[(size_t)lane * 2 + 1] = gh_v; }
    }
    // the lane's report: the latest step at which a non-finite cotangent appeared (the first the sweep met), lowest vehicle -- the
    // maximum of (step, 1023 - vehicle) through one LDS word, off the data path
    int *word = reinterpret_cast<int *>(lds_ck);
    __syncthreads();
    if (k == 0) *word = -1;
    __syncthreads();
    static_assert(DHTS_MICRO_MAX_VEHICLES <= 1024, "the vehicle takes 10 bits of the key");
    if (bad_step >= 0) atomicMax(word, (bad_step << 10) | (1023 - k));
    __syncthreads();
    const int last = *word;
    if (k == 0 && last >= 0) raise_fault(err, DHTS_FAULT_NAN, last >> 10, lane, 1023 - (last & 1023));
}
