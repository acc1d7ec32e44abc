// micro_jvp.inc -- forward-mode tangent sweep (J v) over the IDM rollout tape; included by micro_kernels.hip inside namespace dhts.
//
// The reverse sweep applies the transposes of a step's blocks dEgo = [[1, dt], [e2, e3]] and dLeading = [[0, 0], [-e2, l3]] newest step
// first (micro_rollout_bwd_kernel).  This kernel applies the same blocks untransposed, oldest step first, to kK tangent directions at
// once: the tape entry (e2, e3, l3) of a vehicle-step is read once, the kK tangents ride beside each other.  With (t_pl, t_vl) the
// tangents of the vehicle's leader BEFORE the step and x the parameter term below:
//     t_p' = dot2(1.f, t_p, dtf, t_v)
//     t_v' = (dot2(e2, t_p, e3, t_v) + dot2(-e2, t_pl, l3, t_vl)) + x
// jvp_vehicle is the ONE place that writes this down: every instantiation calls it, so the result of a direction does not depend on how
// many directions ride with it or on its slot among them (bit for bit; tests/test_micro_jvp_gpu.py).  x is the float32 +0.f wherever
// there is no parameter term (no t_params; the acceleration clip), so a call with t_params = 0 returns the bits of the state-only call.
// The head vehicle (slot count - 1) follows the virtual leader (p + head_dp, v - head_dv), the sign convention of the reverse sweep's
// `fold`: t_pl = (float)((double)t_p + t_head[0]), t_vl = (float)((double)t_v - t_head[1]).
//
// kParams: a step also adds x = (float)(dt c), c = sum_q d acc / d theta_q  t_theta_q in double (q = a_max, a_pref, v_target, min_space,
// time_pref in that order, fused multiply-adds; then d acc / d gap  x  -(t_len_leader + t_len) / 2 where the gap is live), the partials
// recomputed by idm_param_jac from the parameter tape's pre-step (p, v) exactly as the kParams reverse sweep recomputes them.
//
// Layout of a launch: directions [0, n_act) of the pointers it is handed, n_act <= kK; the host offsets them by the first direction of
// the launch.  A slot d >= n_act carries zeros and touches no memory (a remainder of three directions rides in a launch of four).
//   t_p_in, t_v_in, t_p_out, t_v_out   [kK][L][V] float32        t_head [kK][L][2] double or NULL       t_params [kK][6][L][V] double
//   t_hist                             [kK][T][L][2][V] float32 or NULL: the tangent of what `hist` holds after every step

__device__ __forceinline__ void jvp_vehicle(const MicroTape3 &c, float dtf, float t_p, float t_v, float t_pl, float t_vl, float x,
                                            float &n_p, float &n_v) {
    n_p = dot2(1.f, t_p, dtf, t_v);
    n_v = (dot2(c.e2, t_p, c.e3, t_v) + dot2(-c.e2, t_pl, c.l3, t_vl)) + x;
}

// the tangents of the head vehicle's virtual leader (p + head_dp, v - head_dv) from the head's own and the head gap's
__device__ __forceinline__ float2 virtual_leader(float t_p, float t_v, double t_head_dp, double t_head_dv) {
    return make_float2((float)((double)t_p + t_head_dp), (float)((double)t_v - t_head_dv));
}

__host__ __device__ inline size_t micro_jvp_lds_bytes(int V, int kK, bool params) {
    return sizeof(float2) * (size_t)(2 * kK + (params ? 2 : 0)) * (size_t)(V + 1) + 2 * sizeof(double) * (size_t)kK;
}

// grid = L workgroups (one traffic lane each) of blockDim.x >= V threads (V rounded up to 64): one vehicle per thread, its kK tangents
// in registers for the whole rollout.  After a step a thread leaves them in TN [copy][direction][slot] for its follower -- the head
// vehicle's thread also leaves those of its virtual leader in the slot behind its own, so every vehicle reads its leader the same
// way --; the two copies alternate with the step parity, so a step takes ONE barrier, and that one waits for LDS only: the tape loads (two steps ahead, clamped
// step index as in the reverse sweep) and the t_hist stores stay in flight across it.  kParams: the pre-step (p, v) of the NEXT step
// travels to the follower the same way (X [copy][slot]), out of the register that was loaded one step earlier.
// The head-gap tangents, which only the head vehicle's thread reads, wait in LDS (TH) instead of 4 kK registers of every thread.
// Dynamic LDS: float2 TN[2][kK][V + 1] | float2 X[2][V + 1] (kParams) | double TH[kK][2]
// A block smaller than the lane, or (kParams) a parameter tape whose header does not name this shape -- it is never read beyond the
// header --: DHTS_FAULT_CAPACITY (index -3), the tangents come back NaN.
template <int kK, bool kParams>
__global__ __launch_bounds__(1024) void micro_rollout_jvp_kernel(
    int L, int V, int T, double dt, const float *__restrict__ tape, const char *__restrict__ ptape, const int32_t *__restrict__ count,
    const double *__restrict__ params, const float *__restrict__ t_p_in, const float *__restrict__ t_v_in,
    const double *__restrict__ t_head, const double *__restrict__ t_params, int n_act,
    float *__restrict__ t_p_out, float *__restrict__ t_v_out, float *__restrict__ t_hist, dhts_error *err) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = blockIdx.x;
    const int k = threadIdx.x;
    const int B = blockDim.x;
    const int P = V + 1;
    float2 *TN = reinterpret_cast<float2 *>(lds);        // [copy][kK][P]
    float2 *X = TN + 2 * kK * P;                         // [copy][P] (kParams)
    double *TH = reinterpret_cast<double *>(TN + (2 * kK + (kParams ? 2 : 0)) * P);      // [kK][2]
    const size_t base = (size_t)lane * V;
    const size_t plane = (size_t)L * V;                  // one direction of a state tangent, one plane of params
    const int nc = count ? count[lane] : V;
    const int n = nc < 0 ? 0 : (nc > V ? V : nc);       // (no slot outside the lane is ever addressed)
    const int Vp = (V + 63) & ~63;
    const bool vk = k < n;
    const bool is_head = k == n - 1;
    const int kc = k < V ? k : 0;
    const float dtf = (float)dt;

    bool ok = V <= B;
    if constexpr (kParams) {
        const ParamTapeHeader h = *reinterpret_cast<const ParamTapeHeader *>(ptape);
        ok = ok && h.magic == kParamTapeMagic && h.L == L && h.V == V && h.T == T;
    }
    if (!ok) {
        const float nanf_ = __builtin_nanf("");
        for (int d = 0; d < n_act; ++d) {
            for (int i = k; i < V; i += B) { t_p_out[d * plane + base + i] = nanf_; t_v_out[d * plane + base + i] = nanf_; }
            if (t_hist)
                for (int s = 0; s < T; ++s)
                    for (int i = k; i < 2 * V; i += B) t_hist[(((size_t)d * T + s) * L + lane) * 2 * V + i] = nanf_;
        }
        if (k == 0) raise_fault(err, DHTS_FAULT_CAPACITY, 0, lane, -3);
        return;
    }

    // this thread's vehicle: its tangents, its parameters and their tangents
    float tp[kK], tv[kK];
#pragma unroll
    for (int d = 0; d < kK; ++d) {
        const bool act = vk && d < n_act;
        tp[d] = act ? t_p_in[d * plane + base + k] : 0.f;
        tv[d] = act ? t_v_in[d * plane + base + k] : 0.f;
    }
    IdmParamDerived pm = {};
    double half_len = 0., head_dp = 0., head_dv = 0.;
    double tth[kParams ? kK : 1][6];                     // t_theta_0 .. 4, then -(t_len_leader + t_len) / 2
    if constexpr (kParams) {
#pragma unroll
        for (int d = 0; d < kK; ++d)
#pragma unroll
            for (int q = 0; q < 6; ++q) tth[d][q] = 0.;
        if (vk) {
            IdmParams raw;
            raw.a_max = params[0 * plane + base + k]; raw.a_pref = params[1 * plane + base + k];
            raw.v_target = params[2 * plane + base + k]; raw.min_space = params[3 * plane + base + k];
            raw.time_pref = params[4 * plane + base + k]; raw.length = params[5 * plane + base + k];
            pm = idm_param_derive(raw);
            const int kl = k + 1 < n ? k + 1 : k;
            half_len = (params[5 * plane + base + kl] + raw.length) * 0.5;
            const double *ph = reinterpret_cast<const double *>(ptape + sizeof(ParamTapeHeader)) + (size_t)lane * 2;
            head_dp = ph[0]; head_dv = ph[1];
#pragma unroll
            for (int d = 0; d < kK; ++d) {
                if (d < n_act) {
                    const double *tq = t_params + (size_t)d * 6 * plane + base;
#pragma unroll
                    for (int q = 0; q < 5; ++q) tth[d][q] = tq[q * plane + k];
                    tth[d][5] = -(tq[5 * plane + kl] + tq[5 * plane + k]) * 0.5;
                }
            }
        }
    }

    for (int i = k; i < (2 * kK + (kParams ? 2 : 0)) * P; i += B) TN[i] = make_float2(0.f, 0.f);
    if (k < 2 * kK) TH[k] = ((k >> 1) < n_act && t_head) ? t_head[((size_t)(k >> 1) * L + lane) * 2 + (k & 1)] : 0.;
    __syncthreads();

    int bad_step = -1;
    if (T > 0) {                                         // (T = 0: no tape to prefetch from -- the tape pointer may be NULL)
        const MicroTape3 *tc0 = reinterpret_cast<const MicroTape3 *>(tape) + (size_t)lane * Vp + kc;
        const size_t step_stride = (size_t)L * Vp;
        MicroTape3 nx = tc0[0];
        MicroTape3 nx2 = tc0[(size_t)(T > 1 ? 1 : 0) * step_stride];
        const float2 *pt0 = nullptr;
        float2 px = make_float2(0.f, 0.f), px2 = px;
        if constexpr (kParams) {
            pt0 = reinterpret_cast<const float2 *>(ptape + param_tape_steps_offset(L)) + (size_t)lane * Vp + kc;
            px = pt0[0]; px2 = pt0[(size_t)(T > 1 ? 1 : 0) * step_stride];
        }
        if (vk) {
#pragma unroll
            for (int d = 0; d < kK; ++d) {
                TN[d * P + k] = make_float2(tp[d], tv[d]);
                if (is_head) TN[d * P + k + 1] = virtual_leader(tp[d], tv[d], TH[2 * d], TH[2 * d + 1]);
            }
            if constexpr (kParams) X[k] = px;
        }
        __syncthreads();
        const size_t h_dir = (size_t)T * L * 2 * V;      // one direction of t_hist
        for (int step = 0; step < T; ++step) {
            const int q = step & 1;
            const MicroTape3 c = nx;
            nx = nx2;
            nx2 = tc0[(size_t)(step + 2 < T ? step + 2 : T - 1) * step_stride];      // two steps ahead
            const float2 cx = px;
            if constexpr (kParams) { px = px2; px2 = pt0[(size_t)(step + 2 < T ? step + 2 : T - 1) * step_stride]; }
            if (vk) {
                // kParams: the partials of this vehicle-step, once for all directions (the collision / clamp rules of the forward,
                // _micro_lane.py:149-166, 201-212, as the kParams reverse sweep rebuilds them)
                IdmParamJac pj = {};
                bool has_x = false, live_gap = false;
                if constexpr (kParams) {
                    const float2 lx = X[q * P + k + 1];
                    const double pv = cx.y;
                    double gap = is_head ? head_dp : fabs((double)lx.x - (double)cx.x) - half_len;
                    double dv = is_head ? head_dv : pv - (double)lx.y;
                    live_gap = !is_head && gap >= 1e-5;      // else a constant: nothing flows to the lengths
                    if (gap < 0) { gap = 0; dv = 0; }
                    gap = (1e-5 > gap) ? 1e-5 : gap;
                    has_x = !(c.e2 == 0.f && c.e3 == 0.f && c.l3 == 0.f);      // (the forward's acceleration clip zeroes all three)
                    if (has_x) idm_param_jac(pv, gap, dv, pm, dt, pj);
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
                    if (is_head) TN[((q ^ 1) * kK + d) * P + k + 1] = virtual_leader(np_, nv_, TH[2 * d], TH[2 * d + 1]);
                    fin = fin && isfinite(np_) && isfinite(nv_);
                }
                if constexpr (kParams) X[(q ^ 1) * P + k] = px;      // what this vehicle enters step + 1 with
                if (bad_step < 0 && !fin) bad_step = step;
            }
            if (t_hist && k < V) {                       // slots at or beyond count: 0 (their tangents never left it)
                float *hp = t_hist + ((size_t)step * L + lane) * 2 * V + k;
#pragma unroll
                for (int d = 0; d < kK; ++d)
                    if (d < n_act) { hp[d * h_dir] = tp[d]; hp[d * h_dir + V] = tv[d]; }
            }
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");     // LDS-only: tape loads and t_hist stores stay in flight
        }
    }
    if (k < V) {
#pragma unroll
        for (int d = 0; d < kK; ++d)
            if (d < n_act) { t_p_out[d * plane + base + k] = tp[d]; t_v_out[d * plane + base + k] = tv[d]; }
    }
    // the lane's EARLIEST non-finite tangent goes on record (a NaN spreads by one vehicle per step: the threads that meet it later must
    // not win the record): the minimum of (step, vehicle) over the workgroup through one LDS word, raised by one thread
    if (err != nullptr) {
        unsigned *word = reinterpret_cast<unsigned *>(lds);
        __syncthreads();
        if (k == 0) *word = 0xffffffffu;
        __syncthreads();
        static_assert(DHTS_MICRO_MAX_VEHICLES <= 1024, "the vehicle takes 10 bits of the key");
        if (bad_step >= 0) atomicMin(word, ((unsigned)(bad_step < (1 << 21) - 1 ? bad_step : (1 << 21) - 1) << 10) | (unsigned)k);
        __syncthreads();
        const unsigned first = *word;
        if (k == 0 && first != 0xffffffffu) raise_fault(err, DHTS_FAULT_NAN, (int)(first >> 10), lane, (int)(first & 1023u));
    }
}
