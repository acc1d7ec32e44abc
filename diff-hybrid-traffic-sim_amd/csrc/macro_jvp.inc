// macro_jvp.inc -- forward-mode tangent sweep (J v) over the rollout tape; included by macro_kernels.hip inside namespace dhts.
//
// The reverse sweeps rebuild the cell blocks dqs[a][0 .. 2] of a step from the tape's interface products (cell_blocks) and apply their
// transposes newest step first.  These kernels apply the same blocks untransposed, oldest step first, to kK tangent directions at once:
// the tape row of a step is read once and its blocks are formed once; the kK tangents ride beside each other.  For cell k of a lane,
// with (d0, d1, d2) row-major 2 x 2 in (r, y), t_{-1} / t_N the tangents of that step's left / right boundary cell:
//     t'_k.r = (dot2(d1.x, t_k.r, d1.y, t_k.y) + dot2(d0.x, t_{k-1}.r, d0.y, t_{k-1}.y)) + dot2(d2.x, t_{k+1}.r, d2.y, t_{k+1}.y)
//     t'_k.y = (dot2(d1.z, t_k.r, d1.w, t_k.y) + dot2(d0.z, t_{k-1}.r, d0.w, t_{k-1}.y)) + dot2(d2.z, t_{k+1}.r, d2.w, t_{k+1}.y)
// jvp_cell below is the ONE place that writes this down: both kernels and every kK call it, so the result of a direction does not depend
// on how many directions ride with it, on its place among them, or on the kernel (bit for bit; tests/test_macro_jvp_gpu.py).
//
// Layout of a launch: directions [0, n_act) of the pointers it is handed, n_act <= kK; the host offsets them by the first direction of the
// launch.  A slot d >= n_act carries zeros and touches no memory (a remainder of three directions rides in a launch of four).
//   t_r_in, t_y_in, t_r_out, t_y_out   [kK][L][N]            (dir_state = L N floats apart; out may alias in: a lane is read whole, then written)
//   t_ghost                            ghost_mode 0: not read (zero) | 1: [kK][L][2][2] | 2: [kK][T][L][2][2], row `step` read by step `step`
//   t_taps                             [kK][T][L][2][n_det]: (t_r, t_y) of the cells det[j] AFTER every step (where the forward writes taps)
// INDEX CONTRACT (the taps form's): det[j] is compared against [0, N) as an unsigned value before any address, LDS or global, is formed
// from it; an entry outside writes nothing.  j is a loop counter < n_det.
// FAULT RECORD: the first step after which a thread finds one of its tangents non-finite raises DHTS_FAULT_NAN (step, lane, cell).

struct JvpBlocks { float4 d0, d1, d2; };
__device__ __forceinline__ void jvp_cell(const JvpBlocks &b, float tlr, float tly, float tr, float ty, float trr, float try_,
                                         float &nr, float &ny) {
    nr = (dot2(b.d1.x, tr, b.d1.y, ty) + dot2(b.d0.x, tlr, b.d0.y, tly)) + dot2(b.d2.x, trr, b.d2.y, try_);
    ny = (dot2(b.d1.z, tr, b.d1.w, ty) + dot2(b.d0.z, tlr, b.d0.w, tly)) + dot2(b.d2.z, trr, b.d2.w, try_);
}

// The lane's EARLIEST non-finite tangent goes on record (a NaN spreads by one cell per step: the threads that meet it later must not
// win the record): the minimum of (step, cell) over the workgroup through one LDS word the kernel no longer needs, raised by one thread.
__device__ __forceinline__ void jvp_raise_first(unsigned *word, int bad_step, int bad_cell, int lane, dhts_error *err) {
    if (err == nullptr) return;
    __syncthreads();
    if (threadIdx.x == 0) *word = 0xffffffffu;
    __syncthreads();
    static_assert(DHTS_MACRO_MAX_CELLS < 4096, "the cell takes 12 bits of the key");
    if (bad_step >= 0) atomicMin(word, ((unsigned)(bad_step < (1 << 20) - 1 ? bad_step : (1 << 20) - 1) << 12) | (unsigned)bad_cell);
    __syncthreads();
    const unsigned first = *word;
    if (threadIdx.x == 0 && first != 0xffffffffu) raise_fault(err, DHTS_FAULT_NAN, (int)(first >> 12), lane, (int)(first & 4095u));
}

// ---- the general kernel: any 1 <= N <= DHTS_MACRO_MAX_CELLS ----------------------------------------------------------------------
// grid = L workgroups (one traffic lane each) of blockDim.x threads (multiple of 64), a strided cell loop as in macro_rollout_bwd_kernel.
// Dynamic LDS: float PL[2 sets][kK][2 (r, y)][N + 2] | u16 SLOT[N + 1].  Index k + 1 of a plane holds cell k; slots 0 and N + 1 hold the
// boundary tangents of the step that reads the set.  A step reads set `step & 1` and writes the other one, so reading the neighbours and
// writing the new value never meet; the detector tangents of a step are read from the set it wrote, behind its barrier.
__host__ __device__ inline size_t jvp_general_lds_bytes(int N, int kK) {
    return sizeof(float) * (size_t)((2 * kK * 2 * (N + 2) + 3) & ~3) + 2 * (size_t)(N + 1);
}
template <int kK>
__global__ __launch_bounds__(512) void macro_rollout_jvp_kernel(
    int L, int N, int T, double cc, const float4 *__restrict__ tape,
    const float *t_r_in, const float *t_y_in, const float *__restrict__ t_ghost, int ghost_mode, int n_act,
    float *t_r_out, float *t_y_out, const int32_t *__restrict__ det, int n_det, float *__restrict__ t_taps, dhts_error *err) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = blockIdx.x;
    const int t = threadIdx.x;
    const int B = blockDim.x;
    const int P = N + 2;
    unsigned short *SLOT = reinterpret_cast<unsigned short *>(lds + ((2 * kK * 2 * P + 3) & ~3));
    const size_t base = (size_t)lane * N;
    const size_t dir_state = (size_t)L * N;
    const size_t dir_ghost = (ghost_mode == 2 ? (size_t)T : 1) * L * 4;
    const size_t dir_taps = (size_t)T * L * 2 * n_det;
    const TapeGeom geo = tape_geom(N);
    const float cf = (float)cc, ncf = (float)(-cc);
    // plane (set q, direction d, component c)
#define DHTS_PL(q_, d_, c_) (lds + (size_t)((((q_) * kK + (d_)) * 2 + (c_)) * P))

    for (int i = t; i < 2 * kK * 2 * P; i += B) lds[i] = 0.f;
    __syncthreads();
    for (int d = 0; d < n_act; ++d)
        for (int k = t; k < N; k += B) {
            DHTS_PL(0, d, 0)[k + 1] = t_r_in[d * dir_state + base + k];
            DHTS_PL(0, d, 1)[k + 1] = t_y_in[d * dir_state + base + k];
        }
    if (ghost_mode == 1 && t < n_act * 4) {          // the same tangent in front of every step: into both sets, once
        const int d = t >> 2, side = (t >> 1) & 1, c = t & 1;
        const float v = t_ghost[d * dir_ghost + (size_t)lane * 4 + (t & 3)];
        DHTS_PL(0, d, c)[side ? N + 1 : 0] = v;
        DHTS_PL(1, d, c)[side ? N + 1 : 0] = v;
    }
    int bad_step = -1, bad_cell = 0;
    for (int step = 0; step < T; ++step) {
        const int q = step & 1;
        const float4 *row = tape + ((size_t)step * L + lane) * geo.row_f4;
        if (ghost_mode == 2 && t < n_act * 4) {      // row `step` of the schedule, into the set this step reads (nobody else touches these slots)
            const int d = t >> 2, side = (t >> 1) & 1, c = t & 1;
            DHTS_PL(q, d, c)[side ? N + 1 : 0] = t_ghost[d * dir_ghost + ((size_t)step * L + lane) * 4 + (t & 3)];
        }
        tape_clear_slots(N, SLOT, t, B);
        __syncthreads();
        tape_fill_slots(row, geo, N, SLOT, t, B);
        __syncthreads();
        for (int k = t; k < N; k += B) {
            float4 aL, bL, aR, bR;
            JvpBlocks b;
            tape_iface(row, geo, N, k, SLOT, aL, bL);
            tape_iface(row, geo, N, k + 1, SLOT, aR, bR);
            cell_blocks(aL, bL, aR, bR, cf, ncf, b.d0, b.d1, b.d2);
            bool fin = true;
#pragma unroll
            for (int d = 0; d < kK; ++d) {
                const float *Tr = DHTS_PL(q, d, 0), *Ty = DHTS_PL(q, d, 1);
                float nr, ny;
                jvp_cell(b, Tr[k], Ty[k], Tr[k + 1], Ty[k + 1], Tr[k + 2], Ty[k + 2], nr, ny);
                DHTS_PL(q ^ 1, d, 0)[k + 1] = nr;
                DHTS_PL(q ^ 1, d, 1)[k + 1] = ny;
                fin = fin && isfinite(nr) && isfinite(ny);
            }
            if (bad_step < 0 && !fin) { bad_step = step; bad_cell = k; }
        }
        __syncthreads();
        if (det) {
            for (int j = t; j < n_det; j += B) {
                const unsigned dc = (unsigned)det[j];
                if (dc < (unsigned)N) {
                    for (int d = 0; d < n_act; ++d) {
                        float *out = t_taps + d * dir_taps + ((size_t)step * L + lane) * 2 * n_det;
                        out[j] = DHTS_PL(q ^ 1, d, 0)[dc + 1];
                        out[n_det + j] = DHTS_PL(q ^ 1, d, 1)[dc + 1];
                    }
                }
            }
        }
    }
    const int qf = T & 1;                          // the set the last step wrote (T = 0: the one that was loaded)
    for (int d = 0; d < n_act; ++d)
        for (int k = t; k < N; k += B) {
            t_r_out[d * dir_state + base + k] = DHTS_PL(qf, d, 0)[k + 1];
            t_y_out[d * dir_state + base + k] = DHTS_PL(qf, d, 1)[k + 1];
        }
#undef DHTS_PL
    jvp_raise_first(reinterpret_cast<unsigned *>(SLOT), bad_step, bad_cell, lane, err);
}

// ---- the fast kernel: one cell per thread, 2 <= N <= kB <= 1024, T > 0 -------------------------------------------------------------
// The shape family of macro_rollout_bwd_fast_kernel.  Thread k owns cell k: the tangents of all kK directions of that cell live in
// registers.  After a step the thread leaves them in TN [copy][direction][k + 1] for its two neighbours (and for the thread that reads a
// detector at that cell); the two copies alternate with the step parity, so a step takes ONE barrier, and that one waits for LDS only:
// the tape loads stay in flight across it.  Slots 0 and N + 1 of a copy hold the boundary tangents of the step that reads it (a constant
// one is written into both copies once; of a schedule, row step + 1 goes into the other copy during step `step`, out of a register that
// was loaded one step earlier).
// Tape: thread k has the trivial products of interfaces k and k + 1 in registers (three floats each, the row's S block); thread j < cnt
// carries exception j to its interface: (A, B) into XA / XB [copy][interface] with the step's tag in STAMP, one interval before the step
// that reads them (a cell whose interface carries the step's tag takes the products from there).  Rows are loaded THREE steps ahead of
// use -- three register sets that trade places in a loop body of three steps --, the exception counts six.
// Detectors: thread j < n_det keeps det[j] in a register and, in the interval after step s, reads the tangents of that cell from the copy
// step s wrote and stores them to row s of t_taps (n_det <= N <= kB: one detector per thread); the last step's row behind one more barrier.
// Dynamic LDS: float4 XA[2][P], XB[2][P] | float2 TN[2][kK][P] | u32 STAMP[2][P]      (P = kB + 2)
__host__ __device__ inline size_t jvp_fast_lds_bytes(int kB, int kK) {
    return 2 * 2 * 16 * (size_t)(kB + 2) + 2 * 8 * (size_t)kK * (kB + 2) + 2 * 4 * (size_t)(kB + 2);
}
template <int kB, int kK>
__global__ __launch_bounds__(kB) __attribute__((amdgpu_waves_per_eu(4, 4))) void macro_rollout_jvp_fast_kernel(     // <= 128 VGPRs
    int L, int N, int T, double cc, const float4 *__restrict__ tape,
    const float *t_r_in, const float *t_y_in, const float *__restrict__ t_ghost, int ghost_mode, int n_act,
    float *t_r_out, float *t_y_out, const int32_t *__restrict__ det, int n_det, float *__restrict__ t_taps, dhts_error *err) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = blockIdx.x;
    const int t = threadIdx.x;
    constexpr int B = kB;
    constexpr int P = kB + 2;
    float4 *XA = reinterpret_cast<float4 *>(lds), *XB = XA + 2 * P;                   // [copy][P]
    float2 *TN = reinterpret_cast<float2 *>(XB + 2 * P);                              // [copy][kK][P]
    unsigned *STAMP = reinterpret_cast<unsigned *>(TN + 2 * kK * P);                  // [copy][P]
    const size_t base = (size_t)lane * N;
    const size_t dir_state = (size_t)L * N;
    const size_t dir_ghost = (ghost_mode == 2 ? (size_t)T : 1) * L * 4;
    const size_t dir_taps = (size_t)T * L * 2 * n_det;
    const TapeGeom geo = tape_geom(N);
    const float cf = (float)cc, ncf = (float)(-cc);
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    const int k = t;
    const bool vk = k < N;
    const int kl = vk ? k : N - 1;
    const int kr = kl + 1 < N ? kl + 1 : N - 1;           // interface N is always an exception: its S entry does not exist
    const size_t row_f4 = geo.row_f4;
    const size_t stride = (size_t)L * row_f4;             // float4s from a lane's row of one step to that of the next
    const float4 *tb = tape + (size_t)lane * row_f4;
    // the detector this thread reads (an entry outside [0, N) matches no cell: -1)
    int det_own = -1;
    if (det && t < n_det) {
        const unsigned dc = (unsigned)det[t];
        if (dc < (unsigned)N) det_own = (int)dc;
    }
    // the boundary tangent this thread carries: (direction t >> 1, side t & 1), (r, y) of it
    const bool bnd = ghost_mode != 0 && t < 2 * kK && (t >> 1) < n_act;
    const int bnd_slot = (t >> 1) * P + ((t & 1) ? N + 1 : 0);
    const float *bnd_src = bnd ? t_ghost + (size_t)(t >> 1) * dir_ghost + (size_t)lane * 4 + 2 * (t & 1) : nullptr;
    const size_t bnd_stride = (size_t)L * 4;

    // a row of the tape: its last one stands in for rows behind the end (loaded, never used)
#define DHTS_ROW(step_) (tb + (size_t)((step_) < T ? (step_) : T - 1) * stride)
#define DHTS_LOAD_CNT(step_, c_) { const unsigned n_ = tape_hdr(DHTS_ROW(step_), geo)[0]; c_ = n_ > (unsigned)N + 1u ? N + 1 : (int)n_; }
#define DHTS_LOAD_S(step_, j_)                                                           \
    {                                                                                    \
        const TapeFp *S_ = reinterpret_cast<const TapeFp *>(DHTS_ROW(step_));            \
        sl[j_] = S_[kl]; sr[j_] = S_[kr];                                                \
    }
#define DHTS_LOAD_E(step_, j_)                                                           \
    if (t < ec[j_]) {                                                                    \
        const float4 *row_ = DHTS_ROW(step_);                                            \
        ix[j_] = tape_idx(tape_hdr(row_, geo), geo)[t];                                  \
        ea[j_] = row_[geo.s_f4 + geo.h_f4 + 2 * t]; eb[j_] = row_[geo.s_f4 + geo.h_f4 + 2 * t + 1]; \
    }
    // more exceptions than threads (the one-phase forward kernel flags every interface): the rest, without prefetch
    auto scatter_rest = [&](int step, int cnt, int q) {
        const float4 *row = DHTS_ROW(step);
        const unsigned short *I = tape_idx(tape_hdr(row, geo), geo);
        const float4 *E = row + geo.s_f4 + geo.h_f4;
        for (int j = t + B; j < cnt; j += B) {             // (cnt <= N + 1: clamped where it is loaded)
            const int i = I[j];
            if (i <= N) { XA[q * P + i] = E[2 * j]; XB[q * P + i] = E[2 * j + 1]; STAMP[q * P + i] = (unsigned)step + 1u; }
        }
    };
    // exception t of step_ (register set j_) to its interface, in LDS copy q_
#define DHTS_SCATTER(step_, q_, j_)                                                      \
    {                                                                                    \
        if (t < ec[j_] && ix[j_] <= (unsigned)N) {                                       \
            XA[(q_) * P + ix[j_]] = ea[j_]; XB[(q_) * P + ix[j_]] = eb[j_]; STAMP[(q_) * P + ix[j_]] = (unsigned)(step_) + 1u; \
        }                                                                                \
        if (ec[j_] > B) scatter_rest(step_, ec[j_], q_);                                 \
    }

    TapeFp sl[3], sr[3];
    float4 ea[3] = {zero4, zero4, zero4}, eb[3] = {zero4, zero4, zero4};
    unsigned ix[3] = {0u, 0u, 0u};
    int ec[3], cq[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) { DHTS_LOAD_CNT(j, ec[j]) DHTS_LOAD_CNT(3 + j, cq[j]) }
#pragma unroll
    for (int j = 0; j < 3; ++j) { DHTS_LOAD_E(j, j) DHTS_LOAD_S(j, j) }

    float tgr[kK], tgy[kK];                      // the own cell's tangents
#pragma unroll
    for (int d = 0; d < kK; ++d) {
        tgr[d] = (vk && d < n_act) ? t_r_in[d * dir_state + base + k] : 0.f;
        tgy[d] = (vk && d < n_act) ? t_y_in[d * dir_state + base + k] : 0.f;
    }
    for (int i = t; i < 2 * P; i += B) STAMP[i] = 0u;
    for (int i = t; i < 2 * kK * P; i += B) TN[i] = make_float2(0.f, 0.f);
    __syncthreads();
    if (vk) {
#pragma unroll
        for (int d = 0; d < kK; ++d) TN[d * P + k + 1] = make_float2(tgr[d], tgy[d]);
    }
    float2 bnd_next = make_float2(0.f, 0.f);     // a schedule: row step + 1, one interval ahead of its store
    if (bnd) {
        const float2 v = *reinterpret_cast<const float2 *>(bnd_src);          // row 0, or the constant tangent
        TN[bnd_slot] = v;
        if (ghost_mode == 1) TN[kK * P + bnd_slot] = v;
        else bnd_next = *reinterpret_cast<const float2 *>(bnd_src + (size_t)(1 < T ? 1 : T - 1) * bnd_stride);
    }
    DHTS_SCATTER(0, 0, 0)
    __syncthreads();

    int bad_step = -1;
    // One barrier interval = one step `st` on register set j_, LDS copy q = st & 1 (read) and q ^ 1 (written):
    //   the blocks of the step (trivial products of set j_, exceptions scattered one interval ago), the neighbours' tangents, the new
    //   tangents and their hand-over; the detector row of step st - 1; the boundary tangents of step st + 1; the exceptions of step
    //   st + 1 (set j_ + 1) to LDS; then the refills: the rest of set j_ for step st + 3, the count of step st + 6.
#define DHTS_STEP(st_, j_)                                                               \
    {                                                                                    \
        const int st = (st_);                                                            \
        const int q = st & 1;                                                            \
        const int oq = q * P;                                                            \
        if (vk) {                                                                        \
            const unsigned tag = (unsigned)st + 1u;                                      \
            const unsigned st0 = STAMP[oq + k], st1 = STAMP[oq + k + 1];                 \
            float4 aL = tape_trivial_A(sl[j_]), bL = zero4, aR = tape_trivial_A(sr[j_]), bR = zero4; \
            if (st0 == tag) { aL = XA[oq + k]; bL = XB[oq + k]; }                        \
            if (st1 == tag) { aR = XA[oq + k + 1]; bR = XB[oq + k + 1]; }                \
            JvpBlocks b;                                                                 \
            cell_blocks(aL, bL, aR, bR, cf, ncf, b.d0, b.d1, b.d2);                      \
            bool fin = true;                                                             \
            _Pragma("unroll") for (int d = 0; d < kK; ++d) {                             \
                const float2 tl = TN[(q * kK + d) * P + k], tr = TN[(q * kK + d) * P + k + 2]; \
                float nr, ny;                                                            \
                jvp_cell(b, tl.x, tl.y, tgr[d], tgy[d], tr.x, tr.y, nr, ny);             \
                tgr[d] = nr; tgy[d] = ny;                                                \
                TN[((q ^ 1) * kK + d) * P + k + 1] = make_float2(nr, ny);                \
                fin = fin && isfinite(nr) && isfinite(ny);                               \
            }                                                                            \
            if (bad_step < 0 && !fin) bad_step = st;                                     \
        }                                                                                \
        if (det_own >= 0 && st >= 1) {                                                   \
            _Pragma("unroll") for (int d = 0; d < kK; ++d) {                             \
                if (d < n_act) {                                                         \
                    const float2 v = TN[(q * kK + d) * P + det_own + 1];                 \
                    float *out = t_taps + d * dir_taps + ((size_t)(st - 1) * L + lane) * 2 * n_det; \
                    out[t] = v.x; out[n_det + t] = v.y;                                  \
                }                                                                        \
            }                                                                            \
        }                                                                                \
        if (ghost_mode == 2 && bnd) {                                                    \
            TN[(q ^ 1) * kK * P + bnd_slot] = bnd_next;                                  \
            bnd_next = *reinterpret_cast<const float2 *>(bnd_src + (size_t)(st + 2 < T ? st + 2 : T - 1) * bnd_stride); \
        }                                                                                \
        if (st + 1 < T) DHTS_SCATTER(st + 1, q ^ 1, ((j_) + 1) % 3)                      \
        ec[j_] = cq[j_];                                                                 \
        DHTS_LOAD_E(st + 3, j_)                                                          \
        DHTS_LOAD_CNT(st + 6, cq[j_])                                                    \
        DHTS_LOAD_S(st + 3, j_)                                                          \
        lds_only_barrier();                                                              \
    }
    int step = 0;
    for (; step + 2 < T; step += 3) {
        DHTS_STEP(step, 0)
        DHTS_STEP(step + 1, 1)
        DHTS_STEP(step + 2, 2)
    }
    if (step < T) DHTS_STEP(step, 0)
    if (step + 1 < T) DHTS_STEP(step + 1, 1)
    if (det_own >= 0) {                          // the row of the last step, from the copy it wrote (behind its barrier)
        const int q = T & 1;
#pragma unroll
        for (int d = 0; d < kK; ++d) {
            if (d < n_act) {
                const float2 v = TN[(q * kK + d) * P + det_own + 1];
                float *out = t_taps + d * dir_taps + ((size_t)(T - 1) * L + lane) * 2 * n_det;
                out[t] = v.x; out[n_det + t] = v.y;
            }
        }
    }
#undef DHTS_STEP
#undef DHTS_SCATTER
#undef DHTS_LOAD_E
#undef DHTS_LOAD_S
#undef DHTS_LOAD_CNT
#undef DHTS_ROW
    if (vk) {
#pragma unroll
        for (int d = 0; d < kK; ++d)
            if (d < n_act) { t_r_out[d * dir_state + base + k] = tgr[d]; t_y_out[d * dir_state + base + k] = tgy[d]; }
    }
    jvp_raise_first(STAMP, bad_step, k, lane, err);
}

// ---- elementwise float32 glue: the tangent maps whose transposes glue_y_bwd / glue_u_bwd (arz_device.hpp) apply ------------------
// y = r (u - u_eq(r)):  t_y = (dy/dr) t_r + (dy/du) t_u with dy/du = r, dy/dr = (u - u_eq) + r u_max 0.5 / sqrt(r + eps) (the last term for
// r >= 0 only: max(r, 0.) picked the constant below)
__device__ __forceinline__ float glue_y_jvp(float r, float u, float um, float t_r, float t_u) {
    float dydr = u - glue_u_eq(r, um);
    if (!(0.f > r)) {
        const float t = r + kEpsF;
        dydr += (r * um) * (0.5f * ((1.f) / (sqrtf(t))));
    }
    return dydr * t_r + r * t_u;
}
// u = y / max(r, eps) + u_eq(max(r, eps)):  t_u = (du/dr) t_r + (du/dy) t_y; below eps the density is the constant eps: du/dr = 0
__device__ __forceinline__ float glue_u_jvp(float r, float y, float um, float t_r, float t_y) {
    if (r < kEpsF) return (t_y) / (kEpsF);
    float dudr = -((((y) / (r))) / (r));
    if (!(0.f > r)) {
        const float t = r + kEpsF;
        dudr += -um * (0.5f * ((1.f) / (sqrtf(t))));
    }
    return dudr * t_r + (t_y) / (r);
}
__global__ void macro_state_from_ru_jvp_kernel(int64_t n, float um, const float *__restrict__ r, const float *__restrict__ u,
                                               const float *__restrict__ t_r, const float *__restrict__ t_u, float *__restrict__ t_y) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        t_y[i] = glue_y_jvp(r[i], u[i], um, t_r[i], t_u[i]);
}
__global__ void macro_u_tap_jvp_kernel(int64_t n, float um, const float *__restrict__ r, const float *__restrict__ y,
                                       const float *__restrict__ t_r, const float *__restrict__ t_y, float *__restrict__ t_u) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        t_u[i] = glue_u_jvp(r[i], y[i], um, t_r[i], t_y[i]);
}
