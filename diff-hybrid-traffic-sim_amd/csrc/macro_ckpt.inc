// macro_ckpt.inc -- reverse mode of the ARZ rollout without a tape in memory: the forward keeps (r, y) of every cell each S steps, the
// reverse sweep replays S steps from a checkpoint with the lane kernel's step, keeps the interface products of every replayed step in an
// LDS ring, sweeps the ring and moves to the checkpoint before; included by macro_kernels.hip inside namespace dhts, after
// macro_fwd_jvp.inc.
//
// What grows with T is the checkpoint buffer alone, float2 [C][L][N] (C = ceil(T / S); row c = the (r, y) every cell of the lane enters
// step c S with): 8 B per cell per S steps against the ~46 B per cell-step of the compact tape.  (u, u_eq) and the cell records of a
// row >= 1 are cell_glue_pre of its (r, y) -- the forward made them that way --; segment 0 replays from the call's own inputs
// (r, y, u, u_eq) with arz_cell_pre, as the forward started, since those are not in general cell_glue_pre of anything.  Row 0 is written
// like every other row and never read.
//
// Arithmetic: the taped pair's own.  The forward and the replay are the two-phase lane kernel's step, statement for statement, as
// macro_fwd_jvp.inc has it (arz_cell_pre, cell_glue_pre, arz_is_trivial_fast, arz_trivial_fast, arz_interface_fast_pre); a trivial
// interface leaves tape_trivial_A(TapeFp{fp[0], fp[2], fp[3]}) and a zero B in the ring, a queued one its (f.A, f.B) -- what
// macro_fwd_jvp.inc keeps in PA / PB and what the compact tape expands to.  The sweep is macro_rollout_bwd_kernel's body on those entries:
// cell_blocks, the detector columns, six dot2, the hand-over (G + c2_left) + c0_right, the boundary addends in double, the NaN record.
// On a ring (kRing) the two hand-over terms that are 0 at the ends of an open lane are read at wrapped slots and no boundary addend exists.
//
// (The dynamic LDS array of the two kernels has a name of its own, smem_ck: block-scope extern declarations of one name are one entity.)
//
// The file is included twice.  DHTS_MACRO_TARGET 0 gives the pair above and the byte helpers; DHTS_MACRO_TARGET 1 the TARGET forms
// (kTarget; dhts_macro_rollout_fwd_ckpt_target / _bwd_ckpt_target), macro_rollout_ckpt_fwd_target_kernel<kP, kBound> and
// macro_rollout_ckpt_bwd_target_kernel<kBound>, from the same text: no detectors (kTaps is false there), `target` [T][L][2][N] -- the
// observed density and speed of every cell after every step, NaN = not observed -- read by the kernels themselves, the forward's sums
// of squared residuals sse [L][2] out and their cotangent g_sse back in.  In the first pass kTarget is false and what the second adds
// sits under it.
//
// kRamp (the last template argument of all four kernels; dhts_macro_rollout_*_ckpt_ramp / _ckpt_target_ramp, DESIGN 4m): a source in
// chosen cells.  ramps [n_ramp] cell indices shared by all lanes, inflow [T][L][n_ramp] the density rate of cell ramps[j] of lane l in
// step t: behind the Godunov update of step t, whose float32 store is unchanged, the owner of the cell forms
// r' = (float)((double)r + dt * (double)inflow[t][l][j]), y' = y, and only then calls the glue, so every reader of "the state after
// step t" -- the next step, the ring's copies, the checkpoint row, the readings, the target residual, the outputs -- sees (r', y).
// The source is identity in (r, y): the sweep is unchanged, and its owner of the cell writes g_inflow[t][l][j] = (float)(dt *
// (double)Gr) from the cotangent in front of step t, behind that row's detector column or target pair.  Row t + 1 of inflow is asked
// for a step ahead of the update that adds it; no barrier in the step loop (the reverse kernel's prologue takes one more, once per
// launch, between writing the columns into the records and their first read), no LDS and no atomic is added.  With kRamp false every kernel is the
// parent's, instruction for instruction but for the offset of one hidden kernel argument.

#if DHTS_MACRO_TARGET == 0
// dynamic LDS: the plan (macro_ckpt_plan) and the kernels' own carving read these
__host__ __device__ inline size_t macro_ckpt_fwd_lds_bytes(int N) { return fwd_jvp_rec_bytes(N); }
// reverse, fixed part: BwdTail, the lane kernel's records and the general sweep's six cotangent planes of N + 2 floats
__host__ __device__ inline size_t macro_ckpt_planes_bytes(int N) { return sizeof(float) * (size_t)((6 * (N + 2) + 3) & ~3); }
// where the lane's output pointers and two row strides wait until they are used: the replay's step leaves no scalar register to carry
// them in, and read back from LDS they arrive in vector registers
struct __attribute__((aligned(16))) BwdTail {
    float *g_r_out, *g_y_out;
    double *g_ghost;
    dhts_error *err;
    ptrdiff_t gt_stride;      // kTaps: floats between two rows of g_taps (read back once per sweep step); kTarget: ... of target
    ptrdiff_t ck_stride;      // float2 entries between two rows of ckpt (once per segment)
};
__host__ __device__ inline size_t macro_ckpt_bwd_fixed_bytes(int N) { return fwd_jvp_rec_bytes(N) + macro_ckpt_planes_bytes(N) + sizeof(BwdTail); }
// ... and per step of the segment ring: (A, B) of the N + 1 interfaces; the target form: and the finished cotangent pair of the N cells
__host__ __device__ inline size_t macro_ckpt_bwd_step_bytes(int N, bool target = false) {
    return 2 * sizeof(float4) * (size_t)(N + 1) + (target ? 2 * sizeof(float) * (size_t)N : 0);
}
__host__ __device__ inline size_t macro_ckpt_bwd_lds_bytes(int N, int S, bool target = false) {
    return macro_ckpt_bwd_fixed_bytes(N) + (size_t)S * macro_ckpt_bwd_step_bytes(N, target);
}
// bytes of one checkpoint row of one lane
__host__ __device__ inline size_t macro_ckpt_row_bytes(int N) { return sizeof(float2) * (size_t)N; }
// kRamp: where a cell's column of ramps[] + 1 waits (0: the cell is no ramp) -- the second half of its record's q0,
// which every step writes as 0. and none reads; the ramp forms write the first half alone.  Looked up by cell, so the replay's owner
// and the sweep's owner of a cell, two threads, read the same word, and neither carries it in a register.  The eight bytes are
// cleared as the double they are declared as (ramp_col_clear); the column goes into and comes out of their first four as bytes
// (memcpy: one 4-byte LDS access, and no object is accessed through a pointer of another type).
__device__ __forceinline__ void ramp_col_clear(CellRec *CR, unsigned cell) { CR[cell + 1].q0.y = 0.; }
__device__ __forceinline__ void ramp_col_set(CellRec *CR, unsigned cell, int col1) { __builtin_memcpy(&CR[cell + 1].q0.y, &col1, sizeof(int)); }
__device__ __forceinline__ int ramp_col_get(const CellRec *CR, unsigned cell) {
    int col1;
    __builtin_memcpy(&col1, &CR[cell + 1].q0.y, sizeof(int));
    return col1;
}
#endif

// grid = L workgroups (one traffic lane each) of W = blockDim.x / 64 wavefronts, the lane kernel's mapping: wave w owns the cells
// [64 kP w, 64 kP (w + 1)), thread t of its pass j the cell 64 kP w + 64 j + t and that cell's LEFT interface.  kP: 64-cell passes per
// wavefront (1 or 2: the plan names no other); kBound: constant boundary cells, a schedule (kSched, as in macro_rollout_fwd2_kernel) or a
// ring (kRing: slots 0 and N + 1 are copies of cells N - 1 and 0, ring_rec_copies in macro_fwd_jvp.inc; DESIGN 4l); kTaps as there.  Two LDS-only barriers per step, the queue
// and the priority rotation as there; no tape and no history.  In phase 1 of step n, n a multiple of Sg, the owner of a cell stores the
// (r, y) the step starts from to row n / Sg of ckpt (consecutive threads, consecutive float2: coalesced).  T >= 1 (the entry point
// copies for T = 0).  At most 12 wavefronts, as macro_rollout_fwd_jvp_kernel: the longest lane the reverse kernel takes has 11.
// err: DHTS_FAULT_CFL (step, lane, interface), as the lane kernel raises it.
// Dynamic LDS: the lane kernel's records (CellRec [N + 2] | flux double2 [N + 1] | queue int [N + 2] | 2 counters).
// kTarget (macro_rollout_ckpt_fwd_target_kernel): in the update the owner of a cell holds the state after step n - 1, row n - 1 of the
// history, and beside it in registers that row's two entries of target, asked for a whole step earlier through a per-thread running
// pointer (no global load on the step's dependent chain); the squared float32 residuals of its valid cells are summed in double in step
// order and combined per lane behind the loop.  ckpt may be NULL: no checkpoint is stored.
#if DHTS_MACRO_TARGET == 0
template <int kP, MacroBoundary kBound, bool kTaps, bool kRamp>
__global__ __launch_bounds__(768) void macro_rollout_ckpt_fwd_kernel(
#else
template <int kP, MacroBoundary kBound, bool kRamp>
__global__ __launch_bounds__(768) void macro_rollout_ckpt_fwd_target_kernel(
#endif
    int L, int N, int T, int Sg, double dt, double dx, double um,
    const float *__restrict__ r_in, const float *__restrict__ y_in, const float *__restrict__ u_in,
    const float *__restrict__ q_in, const float *__restrict__ ghost,
    float *__restrict__ r_out, float *__restrict__ y_out, float *__restrict__ u_out, float *__restrict__ q_out,
    float2 *__restrict__ ckpt, dhts_error *err,
#if DHTS_MACRO_TARGET == 0
    const int32_t *__restrict__ det, int n_det, float *__restrict__ taps,
    const int32_t *__restrict__ ramps, int n_ramp, const float *__restrict__ inflow) {
    constexpr bool kTarget = false;
    const float *const target = nullptr;
    double *const sse = nullptr;
#else
    const float *__restrict__ target, double *__restrict__ sse,
    const int32_t *__restrict__ ramps, int n_ramp, const float *__restrict__ inflow) {
    constexpr bool kTaps = false, kTarget = true;
    const int32_t *const det = nullptr;
    constexpr int n_det = 0;
    float *const taps = nullptr;
#endif
    constexpr bool kSched = kBound == kBoundSched, kRing = kBound == kBoundRing;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_ck[];
    const int lane = blockIdx.x;
    const int tid = threadIdx.x;
    const int t = tid & 63;
    const int wv = tid >> 6;
    const int Wc = blockDim.x >> 6;                  // wavefronts
    const int ncell = blockDim.x;
    const size_t base = (size_t)lane * N;
    CellRec *CR = reinterpret_cast<CellRec *>(smem_ck);
    double2 *FX = reinterpret_cast<double2 *>(CR + (N + 2));
    int *Q = reinterpret_cast<int *>(FX + (N + 1));
    int *CNT = Q + (N + 2);                          // queue length by step parity
    IfaceConst kc;
    kc.set_um(um); kc.set_grid(dt, dx);

    for (int k = tid; k < N + 2; k += blockDim.x) {
        float4 st;
        if (kRing && (k == 0 || k == N + 1)) {           // a ring: slot 0 is cell N - 1, slot N + 1 is cell 0
            const size_t w = base + (k ? 0 : N - 1);
            st = make_float4(r_in[w], y_in[w], u_in[w], q_in[w]);
        } else if (k == 0 || k == N + 1) {
            const float *g = ghost + (size_t)lane * 8 + (k ? 4 : 0);
            st = make_float4(g[0], g[1], g[2], g[3]);
        } else {
            st = make_float4(r_in[base + k - 1], y_in[base + k - 1], u_in[base + k - 1], q_in[base + k - 1]);
        }
        CellPre c;
        arz_cell_pre((double)st.x, um, c);
        CR[k].st = st;
        CR[k].sh = make_double2(c.s, c.h);
        CR[k].q0 = make_double2(c.q0, 0.);
    }
    if (tid == 0) { Q[0] = N; CNT[0] = 1; CNT[1] = 1; }      // entry 0 of every step's queue: interface N
    __syncthreads();

    const int lo = wv * (kP << 6);                   // first cell of this wave
    const double c = dt / dx;                        // update_coefficient, _macro_lane.py:99
    const float umf = (float)um;
    int fault_step = -1, fault_index = 0;
    int rot = 0;                                     // the cell wave that takes the head of the queue rotates with the step
    double rd_own[kP], yd_own[kP];                   // (r, y) of the thread's own cells, carried from step to step

    float2 *ck_row = ckpt + base;                    // this lane's part of the next row to fill; a row is L N entries
    const size_t ck_stride = (size_t)L * N;
    int next_ck = 0;

    float4 sched_st = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 *sched_p = nullptr;
    if constexpr (kSched) {
        sched_p = reinterpret_cast<const float4 *>(ghost) + ((size_t)L + lane) * 2 + (tid & 1);
        if (tid < 2 && T > 1) sched_st = *sched_p;
    }
    // kTarget: this thread's cells in the row of target that is loaded next (running pointers; a row is L 2 N floats, the speed plane
    // N floats behind the density plane), the row the next update is held against, and the thread's two sums
    const float *tgp[kP];
    float tg_r[kP], tg_u[kP];
    double sse_r = 0., sse_u = 0.;
    if constexpr (kTarget) {
#pragma unroll
        for (int j = 0; j < kP; ++j) {
            const int i = lo + (j << 6) + t;
            tgp[j] = target + (size_t)lane * 2 * N + (i < N ? i : N - 1);
            tg_r[j] = tgp[j][0]; tg_u[j] = tgp[j][N];
        }
    }
    // kRamp: thread q puts column q + 1 of ramps[q] into that cell's record once (ramp_col_set: the word the reverse kernel uses; an
    // entry outside [0, N) is compared as an unsigned value and forms no address), so the owner of a cell finds its column with the
    // record it updates and carries none.  src[j]: the entry of the row of inflow the next update adds, asked for a whole step earlier;
    // the row's address is formed from the step count where it is loaded.  The ramp forms write the first half of q0 alone.
    float src[kP];
    const float *const rin = kRamp ? inflow + (size_t)lane * n_ramp : nullptr;      // this lane's part of row 0
    if constexpr (kRamp) {
        for (int q = tid; q < n_ramp; q += blockDim.x) {
            const unsigned rc = (unsigned)ramps[q];
            if (rc < (unsigned)N) ramp_col_set(CR, rc, q + 1);
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kP; ++j) {
            const int i = lo + (j << 6) + t;
            const int rc = i < N ? ramp_col_get(CR, (unsigned)i) : 0;
            src[j] = rc ? rin[rc - 1] : 0.f;
        }
    }
    // kTaps: thread (blockDim - 1 - tid) takes detector slot tap_j (+ blockDim per further one); tap_wave: this wavefront holds any
    const int tap_j = (int)blockDim.x - 1 - tid;
    int det_own = -1;
    bool tap_wave = false;
    if constexpr (kTaps) {
        tap_wave = __builtin_amdgcn_readfirstlane((Wc - 1 - wv) << 6) < n_det;
        if (tap_j < n_det) det_own = det[tap_j];
    }
    auto tap = [&](const int s) {                       // the state after step s, out of the records
        if (tap_wave) {
            const CellRec *cr = CR;
            taps_write(det, n_det, det_own, tap_j, (int)blockDim.x, N, taps + ((size_t)s * L + lane) * 3 * n_det,
                       [=](unsigned dc) { return cr[dc + 1].st; });
        }
    };

    auto body = [&](auto upd_c, auto solve_c, const int n) {
        constexpr bool upd = decltype(upd_c)::value;       // finish step n - 1
        constexpr bool solve = decltype(solve_c)::value;   // start step n
        if constexpr (kSched && upd && solve) {
            if (tid < 2) {
                CellPre cg;
                arz_cell_pre((double)sched_st.x, um, cg);
                CellRec *gr = CR + (tid ? N + 1 : 0);
                gr->st = sched_st; gr->sh = make_double2(cg.s, cg.h); gr->q0 = make_double2(cg.q0, 0.);
                sched_p += (size_t)L * 2;
                if (n + 1 < T) sched_st = *sched_p;
            }
        }
        const bool ck_now = solve && n == next_ck;         // step n starts a segment: its (r, y) go to the next row
        int *cnt = CNT + (n & 1);
#pragma unroll
        for (int j = 0; j < kP; ++j) {
            const int i = lo + (j << 6) + t;                // cell i and its left interface i
            const bool vc = i < N;
            const unsigned ic = (unsigned)(vc ? i : N - 1);
            CellRec *own = CR + ic + 1;
            float4 st;
            if (!upd) { st = own->st; rd_own[j] = (double)st.x; yd_own[j] = (double)st.y; }
            if (upd) {
                // Godunov update, _macro_lane.py:109-112, float32 store :327-334
                const double2 Fl = FX[ic], Fr = FX[ic + 1];
                st.x = (float)(rd_own[j] + (Fl.x - Fr.x) * c);
                st.y = (float)(yd_own[j] + (Fl.y - Fr.y) * c);
                if constexpr (kRamp) {
                    // the on-ramp's source of step n - 1, one more float32 operation behind the step's own store (DESIGN 4m); then
                    // row n leaves for the register
                    const int rc = vc ? ramp_col_get(CR, ic) : 0;
                    if (rc) {
                        st.x = (float)((double)st.x + dt * (double)src[j]);
                        if (solve) src[j] = rin[(size_t)n * L * n_ramp + (rc - 1)];
                    }
                }
                rd_own[j] = (double)st.x; yd_own[j] = (double)st.y;
                CellPre cp;
                cell_glue_pre(st.x, st.y, umf, kc, st.z, st.w, cp);     // set_next_state_vector_y, :282-299
                if (vc && solve) {
                    own->st = st; own->sh = make_double2(cp.s, cp.h);
                    if constexpr (kRamp) own->q0.x = cp.q0; else own->q0 = make_double2(cp.q0, 0.);
                }
                else if (kTaps && vc) own->st = st;          // the final step's state, for the taps below
                if constexpr (kRing && solve) ring_rec_copies_direct(CR, N, vc, ic, st, cp);
                if constexpr (kTarget) {
                    // st is row n - 1 of the history: the float32 residuals against that row of target (NaN: not observed), squared
                    // and summed in double; then row n leaves for the registers, a whole step ahead of the update that reads it
                    const float er = isnan(tg_r[j]) ? 0.f : st.x - tg_r[j];
                    const float eu = isnan(tg_u[j]) ? 0.f : st.z - tg_u[j];
                    if (vc) { sse_r += (double)er * (double)er; sse_u += (double)eu * (double)eu; }
                    if (solve) { tgp[j] += (size_t)L * 2 * N; tg_r[j] = tgp[j][0]; tg_u[j] = tgp[j][N]; }
                }
            }
            if (!solve) {
                if (vc) { r_out[base + i] = st.x; y_out[base + i] = st.y; u_out[base + i] = st.z; q_out[base + i] = st.w; }
                continue;
            }
            if (ck_now && vc && (!kTarget || ckpt)) ck_row[i] = make_float2(st.x, st.y);
            // the left neighbour at this time level: written just above by the lane below, or in the previous pass (a wave's
            // LDS operations complete in order); the first cell of the chunk has its left neighbour in another wave: queued
            wave_lds_handoff();
            const CellRec *lf = CR + ic;
            const float4 ls = lf->st;
            const double2 lsh = lf->sh, lq0 = lf->q0;
            CellPre cl;
            cl.s = lsh.x; cl.h = lsh.y; cl.q0 = lq0.x;
            IfacePre pre;
            const bool easy = arz_is_trivial_fast((double)ls.x, (double)ls.z, (double)ls.w, (double)st.x, (double)st.z, cl, kc, pre);
            const bool triv = vc & easy & !((j == 0) & (t == 0));
            double u0, Fr, Fy;
            float fp[4];
            arz_trivial_fast((double)ls.x, (double)ls.y, pre, kc, u0, Fr, Fy, fp);
            if (triv) FX[ic] = make_double2(Fr, Fy);
            const bool nt = vc & !triv;
            if (nt) Q[atomicAdd(cnt, 1)] = i;
        }
        if (!solve) {
            if constexpr (kTaps && upd) { lds_only_barrier(); tap(n - 1); }
            return;
        }
        if (ck_now) { ck_row += ck_stride; next_ck += Sg; }
        lds_only_barrier();
        // ---- phase 2: the queued interfaces ----
        int k0 = tid - (rot << 6);
        if (k0 < 0) k0 += ncell;
        const unsigned i_q = (unsigned)Q[k0 <= N ? k0 : 0];  // read beside the count, not behind it (one LDS round trip less)
        const int qn = *cnt;
        if (k0 < qn) __builtin_amdgcn_s_setprio(3);          // the workgroup's critical path
        for (int k = k0; k < qn; k += ncell) {
            const unsigned i = (k == k0) ? i_q : (unsigned)Q[k];
            const CellRec *lf = CR + i, *rt = CR + i + 1;
            const float4 ls = lf->st, rs = rt->st;
            const double2 lsh = lf->sh, lq0 = lf->q0, rsh = rt->sh;
            CellPre cl, cr;
            cl.s = lsh.x; cl.h = lsh.y; cl.q0 = lq0.x;
            cr.s = rsh.x; cr.h = rsh.y; cr.q0 = 0.;
            Iface f;
            arz_interface_fast_pre((double)ls.x, (double)ls.y, (double)ls.z, (double)ls.w, cl,
                                   (double)rs.x, (double)rs.y, (double)rs.z, (double)rs.w, cr, kc, f);
            FX[i] = make_double2(f.Fr, f.Fy);
            if (f.cfl_bad && fault_step < 0) { fault_step = n; fault_index = (kRing && i == (unsigned)N) ? 0 : (int)i; }      // (a ring: N is 0)
        }
        __builtin_amdgcn_s_setprio(0);
        if constexpr (kTaps && upd) tap(n - 1);
        if (tid == 0) CNT[(n + 1) & 1] = 1;
        if (++rot == Wc) rot = 0;
        lds_only_barrier();
    };
    using yes = std::integral_constant<bool, true>;
    using no = std::integral_constant<bool, false>;
    body(no{}, yes{}, 0);
    for (int n = 1; n < T; ++n) body(yes{}, yes{}, n);
    body(yes{}, no{}, T);
    if (fault_step >= 0) raise_fault(err, DHTS_FAULT_CFL, fault_step, lane, fault_index);
    if constexpr (kTarget) {
        // the lane's two sums: over the wavefront by the butterfly 32, 16 .. 1, then thread 0 over the wavefronts in their order, through
        // the LDS the step loop is done with -- one fixed tree for a given launch shape, no atomics
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { sse_r += __shfl_xor(sse_r, o); sse_u += __shfl_xor(sse_u, o); }
        __syncthreads();
        double2 *part = reinterpret_cast<double2 *>(smem_ck);
        if (t == 0) part[wv] = make_double2(sse_r, sse_u);
        __syncthreads();
        if (tid == 0) {
            double2 a = part[0];
            for (int w = 1; w < Wc; ++w) { a.x += part[w].x; a.y += part[w].y; }
            sse[(size_t)lane * 2] = a.x; sse[(size_t)lane * 2 + 1] = a.y;
        }
    }
}

// grid = L workgroups of the forward's W wavefronts, the same mapping.  Dynamic LDS (macro_ckpt_bwd_lds_bytes):
//   BwdTail                                                      the lane's output pointers (above)
//   the lane kernel's records (fwd_jvp_rec_bytes(N))            the replay's
//   float4 R[Sg][2][N + 1]                                       the ring: (A, B) of interface i of step r of the segment at R[r][0 / 1][i]
//   float  Gr, Gy, C0r, C0y, C2r, C2y [N + 2]                    the general sweep's cotangent planes (bwd_planes)
// Segments seg = C - 1 .. 0: the owner of a cell writes its record from row seg of ckpt (in registers since the segment after this one
// was started: the load is in flight across that segment's replay and sweep; every barrier waits for LDS only) -- cell_glue_pre of the
// row's (r, y); segment 0: the call's inputs with arz_cell_pre --, threads 0 and 1 the boundary records (of a schedule: row seg Sg), and
// the steps [seg Sg, min(T, (seg + 1) Sg)) are replayed with the forward's loop, without its last update: the products of step n are
// complete behind phase 2 of step n.  The replay raises no CFL fault (the forward did), writes no readings, and with a schedule reads
// the boundary rows of its steps again.  Then the segment is swept newest first out of the ring with macro_rollout_bwd_kernel's body,
// the strided cell loop included.
// p: the forward's 64-cell passes per wavefront, a run-time value here (the replay's step unrolled over two passes leaves neither scalar
// nor vector registers for the sweep: it spilled both).
// kTaps: the detector columns are added by the OWNER of the cell, behind the hand-over that precedes the step they go in front of --
// macro_rollout_bwd_kernel's Gr[det[j] + 1] += gt[j] on the same operands, without a pass and a barrier of its own.
// Barriers: the replay takes the lane kernel's two per step.  Of the taped sweep's four per step the two around the slot table have
// nothing to order here; TWO remain (cell loop -> hand-over, hand-over -> next cell loop), with and without detectors.
// Scalar registers: the replay's step takes about 100 of the 106 by itself, so what the sweep walks (ckpt, g_taps, g_ghost, the
// schedule) goes through per-thread running pointers in vector registers, and BwdTail holds what is needed once.
// err: DHTS_FAULT_NAN as macro_rollout_bwd_kernel raises it (every thread reports the first non-finite cotangent it met: the latest step).
// kTarget (macro_rollout_ckpt_bwd_target_kernel; it excludes kTaps): the per-step cotangent is that of sse, formed here.  The replay of
// step n holds, in its update (the checkpoint's record for n = s0), the state (r, y, u) after step n - 1 = row n - 1 of the history: its
// owner loads that row of target at the top of the pass, and at the bottom forms gr = g2r (r - t_r), gy = 0, glue_u_bwd(r, y, um,
// g2u (u - t_u), gr, gy) -- g2r, g2u = (float)(2 g_sse[lane][0 / 1]), a NaN entry's residual 0: the float32 operations of the dense
// path's glue on a dense g_hist -- and leaves the pair in two more float planes of the ring, TP[n - s0][0 / 1][cell], since the replay's
// owner of a cell is not the sweep's.  The sweep adds the pair of row step - 1 behind the hand-over of step, where the columns of kTaps go.
// Row T - 1 is the forward's final state, which the caller has: fin_r, fin_y, fin_u are read once in front of the loop and the pair goes
// into the incoming cotangent, as the last row of g_taps does.  The sweep itself takes no global load beyond what it has.
#if DHTS_MACRO_TARGET == 0
template <MacroBoundary kBound, bool kTaps, bool kRamp>
__global__ __launch_bounds__(768) void macro_rollout_ckpt_bwd_kernel(
#else
template <MacroBoundary kBound, bool kRamp>
__global__ __launch_bounds__(768) void macro_rollout_ckpt_bwd_target_kernel(
#endif
    int L, int N, int T, int Sg, int p, double dt, double dx, double um, const float2 *__restrict__ ckpt,
    const float *__restrict__ r_in, const float *__restrict__ y_in, const float *__restrict__ u_in,
    const float *__restrict__ q_in, const float *__restrict__ ghost,
    const float *__restrict__ g_r_in, const float *__restrict__ g_y_in, const float *__restrict__ g_taps,
    float *__restrict__ g_r_out, float *__restrict__ g_y_out, double *__restrict__ g_ghost, dhts_error *err,
#if DHTS_MACRO_TARGET == 0
    const int32_t *__restrict__ det, int n_det,
    const int32_t *__restrict__ ramps, int n_ramp, const float *__restrict__ inflow, float *__restrict__ g_inflow) {
    constexpr bool kTarget = false;
    const float *const target = nullptr, *const fin_r = nullptr, *const fin_y = nullptr, *const fin_u = nullptr;
    const double *const g_sse = nullptr;
#else
    const float *__restrict__ target, const double *__restrict__ g_sse,
    const float *__restrict__ fin_r, const float *__restrict__ fin_y, const float *__restrict__ fin_u,
    const int32_t *__restrict__ ramps, int n_ramp, const float *__restrict__ inflow, float *__restrict__ g_inflow) {
    constexpr bool kTaps = false, kTarget = true;
    const int32_t *const det = nullptr;
    constexpr int n_det = 0;
#endif
    constexpr bool kSched = kBound == kBoundSched, kRing = kBound == kBoundRing;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_ck[];
    const int lane = blockIdx.x;
    const int tid = threadIdx.x;
    const int t = tid & 63;
    const int wv = tid >> 6;
    const int Wc = blockDim.x >> 6;
    const int ncell = blockDim.x;
    const int B = blockDim.x;
    const int P = N + 2;
    const size_t base = (size_t)lane * N;
    BwdTail *tail = reinterpret_cast<BwdTail *>(smem_ck);       // at a literal address: no register holds it
    CellRec *CR = reinterpret_cast<CellRec *>(smem_ck + sizeof(BwdTail));
    double2 *FX = reinterpret_cast<double2 *>(CR + (N + 2));
    int *Q = reinterpret_cast<int *>(FX + (N + 1));
    int *CNT = Q + (N + 2);
    float4 *R = reinterpret_cast<float4 *>(smem_ck + sizeof(BwdTail) + fwd_jvp_rec_bytes(N));
    const BwdPlanes pl = bwd_planes(reinterpret_cast<float *>(R + (size_t)Sg * 2 * (N + 1)), P);
    float *Gr = pl.Gr, *Gy = pl.Gy, *C0r = pl.C0r, *C0y = pl.C0y, *C2r = pl.C2r, *C2y = pl.C2y;
    IfaceConst kc;
    kc.set_um(um); kc.set_grid(dt, dx);

    // kTarget: the cotangent pairs of the ring, float TP[Sg][2][N] behind the planes (macro_ckpt_bwd_step_bytes(N, true) per step in all)
    float *const TP = pl.Gr + ((6 * P + 3) & ~3);
    if (tid == 0) *tail = BwdTail{g_r_out + base, g_y_out + base, g_ghost ? g_ghost + (size_t)lane * 4 : nullptr, err,
                                   kTarget ? (ptrdiff_t)L * 2 * N : (ptrdiff_t)L * 2 * n_det, (ptrdiff_t)L * N};
    for (int k = tid; k < P; k += B) { C0r[k] = 0.f; C0y[k] = 0.f; C2r[k] = 0.f; C2y[k] = 0.f; Gr[k] = 0.f; Gy[k] = 0.f; }
    if constexpr (kRamp)
        for (int k = tid; k < N; k += B) ramp_col_clear(CR, (unsigned)k);
    __syncthreads();
    // kTaps: the sweep's owner of cell k = tid + m B (2 B >= N) adds the detector columns to it itself, so it looks its cells up in
    // det[] once: col[m] = the column j with det[j] == k, -1 without one (an entry outside [0, N) matches no cell; it is compared as an
    // unsigned value and forms no address).  gtp[m]: that column in the row of g_taps which is added next, a per-thread running pointer.
    // PRECONDITION: the entries of det inside [0, N) are distinct (include/dhts.h).  One column per cell is kept, the last match, where
    // macro_rollout_bwd_kernel adds every column that names the cell: with a repeated entry the two sweeps differ.
    int col[2];
    const float *gtp[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) { col[m] = -1; gtp[m] = nullptr; }
    if constexpr (kTaps) {
        for (int j = 0; j < n_det; ++j) {
            const unsigned dc = (unsigned)det[j];
#pragma unroll
            for (int m = 0; m < 2; ++m)
                if (dc < (unsigned)N && dc == (unsigned)(tid + m * B)) col[m] = j;
        }
#pragma unroll
        for (int m = 0; m < 2; ++m) gtp[m] = g_taps + ((size_t)(T - 1) * L + lane) * 2 * n_det + (col[m] >= 0 ? col[m] : 0);
    }
    // kRamp: the owner of a ramp cell, in the replay and in the sweep, finds the cell's column in the records (ramp_col_get): thread q writes
    // column q + 1 there once, here.  An entry of ramps outside [0, N) is compared as an unsigned value and forms no address; with a
    // repeated entry one of its columns stays (PRECONDITION, include/dhts.h).  src0 / src1: the replay's entries of inflow for its pass
    // 0 / 1, asked for a whole step ahead of the update that adds them.  The rows of inflow and g_inflow are addressed from the step
    // count where they are used: that is scalar work, and no running pointer is carried.
    float src0 = 0.f, src1 = 0.f;
    if constexpr (kRamp) {
        for (int q = tid; q < n_ramp; q += B) {          // (the words were cleared in front of the barrier above)
            const unsigned rc = (unsigned)ramps[q];
            if (rc < (unsigned)N) ramp_col_set(CR, rc, q + 1);
        }
        __syncthreads();
    }
    const float *const rin = kRamp ? inflow + (size_t)lane * n_ramp : nullptr;      // this lane's part of row 0
    float *const gin = kRamp ? g_inflow + (size_t)lane * n_ramp : nullptr;
    // kTarget: twice the cotangent of the lane's two sums, in float32 (per thread: the scalar registers are the replay's)
    float g2r = 0.f, g2u = 0.f;
    if constexpr (kTarget) {
        g2r = (float)(2. * g_sse[(size_t)lane * 2]); g2u = (float)(2. * g_sse[(size_t)lane * 2 + 1]);
        asm volatile("" : "+v"(g2r), "+v"(g2u));         // (held in vector registers from here on)
    }
    // the cotangent pair of one history row at one cell, from the state (r, y, u) there and the row's two entries of target
    auto fit_pair = [&](const float r, const float y, const float u, const float t_r, const float t_u, float &gr, float &gy) {
        gr = isnan(t_r) ? 0.f : g2r * (r - t_r);
        gy = 0.f;
        glue_u_bwd(r, y, (float)um, isnan(t_u) ? 0.f : g2u * (u - t_u), gr, gy);
    };
    // the cotangent of the final state, and in front of step T - 1 its detector columns (macro_rollout_bwd_kernel: Gr[det[j] + 1] += gt[j])
    // resp. (kTarget) the pair of row T - 1, from the forward's final state
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const int k = tid + m * B;
        if (k < N) {
            float gr = g_r_in[base + k], gy = g_y_in[base + k];
            if (kTaps && col[m] >= 0) { gr += gtp[m][0]; gy += gtp[m][n_det]; }
            if constexpr (kTarget) {
                const float *tg = target + ((size_t)(T - 1) * L + lane) * 2 * N + k;
                float ar, ay;
                fit_pair(fin_r[base + k], fin_y[base + k], fin_u[base + k], tg[0], tg[N], ar, ay);
                gr += ar; gy += ay;
            }
            if constexpr (kRamp) {                       // row T - 1: the source is identity in (r, y)
                const int rc = ramp_col_get(CR, (unsigned)k);
                if (rc) gin[(size_t)(T - 1) * L * n_ramp + (rc - 1)] = (float)(dt * (double)gr);
            }
            Gr[k + 1] = gr; Gy[k + 1] = gy;
        }
    }
    __syncthreads();

    if constexpr (kTarget) __builtin_assume(p >= 1 && p <= 2);      // (the plan names no other: the pass loops' entry tests hold no scalar registers)
    const int lo = wv * (p << 6);
    const double c = dt / dx;
    const float cf = (float)c, ncf = (float)(-c);
    const float umf = (float)um;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    int rot = 0;
    const int Nv = kRing ? ring_len(N) : N;          // (a ring: see ring_rec_copies)
    float4 sched_st = zero4;
    const float4 *sched_p = nullptr;
    // kSched: this lane's boundary cell (tid & 1) of row 0 of the schedule (a per-thread pointer: threads 0 and 1 use it)
    const float4 *sched_lane = reinterpret_cast<const float4 *>(ghost) + (size_t)lane * 2 + (tid & 1);

    // kSched: entry (tid & 1) of the row of g_ghost the sweep is at, likewise
    double2 *gs_run = nullptr;
    if constexpr (kSched) gs_run = reinterpret_cast<double2 *>(g_ghost) + ((size_t)(T - 1) * L + lane) * 2 + (tid & 1);

    double ghl_r = 0., ghl_y = 0., ghr_r = 0., ghr_y = 0.;   // ghost cotangent sums (thread 0 / thread of cell N-1)
    int bad_step = -1, bad_cell = 0;     // first non-finite cotangent this thread meets (the reverse sweep's first = the latest step)
    // kTarget: the thread's first cell in the row of target the replay reads next (a per-thread running pointer), and where the pairs of
    // that step go in the ring
    const int own0 = lo + t;
    const float *tg_run = nullptr;
    float *tp0 = TP + own0;              // (per thread, and opaque to the compiler from here on: a vector register, like g2r / g2u)
    if constexpr (kTarget) asm volatile("" : "+v"(tp0));
    float *tp_run = tp0;

    // the replay of step n, s_end = one past the segment's last step; RA / RB = the ring entry of step n
    auto body = [&](auto upd_c, const int n, const int s_end, float4 *RA, float4 *RB) {
        constexpr bool upd = decltype(upd_c)::value;       // finish step n - 1
        if constexpr (kSched && upd) {
            if (tid < 2) {
                CellPre cg;
                arz_cell_pre((double)sched_st.x, um, cg);
                CellRec *gr = CR + (tid ? N + 1 : 0);
                gr->st = sched_st; gr->sh = make_double2(cg.s, cg.h); gr->q0 = make_double2(cg.q0, 0.);
                sched_p += (size_t)L * 2;
                if (n + 1 < s_end) sched_st = *sched_p;
            }
        }
        int *cnt = CNT + (n & 1);
#pragma unroll 1
        for (int j = 0; j < p; ++j) {
            const int i = lo + (j << 6) + t;                // cell i and its left interface i
            const bool vc = i < N;
            const unsigned ic = (unsigned)(vc ? i : N - 1);
            CellRec *own = CR + ic + 1;
            float4 st = own->st;
            int rsj = 0;
            if constexpr (kRamp && upd) rsj = vc ? ramp_col_get(CR, ic) : 0;
            // kTarget: row n - 1 of target at this cell, asked for here and used at the bottom of the pass
            float t_r = 0.f, t_u = 0.f;
            if constexpr (kTarget) {
                if (n > 0) { const float *tg = tg_run + ((int)ic - own0); t_r = tg[0]; t_u = tg[N]; }
            }
            if (upd) {
                // Godunov update, _macro_lane.py:109-112, float32 store :327-334
                const double2 Fl = FX[ic], Fr = FX[ic + 1];
                st.x = (float)((double)st.x + (Fl.x - Fr.x) * c);
                st.y = (float)((double)st.y + (Fl.y - Fr.y) * c);
                if constexpr (kRamp) {
                    // the forward's float32 source of step n - 1 on the same operands; then row n leaves for the register
                    if (rsj) {
                        st.x = (float)((double)st.x + dt * (double)(j ? src1 : src0));
                        if (n + 1 < s_end) {
                            const float nx = rin[(size_t)n * L * n_ramp + (rsj - 1)];
                            if (j) src1 = nx; else src0 = nx;
                        }
                    }
                }
                CellPre cp;
                cell_glue_pre(st.x, st.y, umf, kc, st.z, st.w, cp);     // set_next_state_vector_y, :282-299
                if (vc) {
                    own->st = st; own->sh = make_double2(cp.s, cp.h);
                    if constexpr (kRamp) own->q0.x = cp.q0; else own->q0 = make_double2(cp.q0, 0.);
                }
                if constexpr (kRing) ring_rec_copies<kRamp>(CR, Nv, vc, ic, st, cp);
            }
            wave_lds_handoff();
            const CellRec *lf = CR + ic;
            const float4 ls = lf->st;
            const double2 lsh = lf->sh, lq0 = lf->q0;
            CellPre cl;
            cl.s = lsh.x; cl.h = lsh.y; cl.q0 = lq0.x;
            IfacePre pre;
            const bool easy = arz_is_trivial_fast((double)ls.x, (double)ls.z, (double)ls.w, (double)st.x, (double)st.z, cl, kc, pre);
            const bool triv = vc & easy & !((j == 0) & (t == 0));
            double u0, Fr, Fy;
            float fp[4];
            arz_trivial_fast((double)ls.x, (double)ls.y, pre, kc, u0, Fr, Fy, fp);
            if (triv) {
                FX[ic] = make_double2(Fr, Fy);
                RA[ic] = tape_trivial_A(TapeFp{fp[0], fp[2], fp[3]});      // what the lane kernel's tape entry expands to
                RB[ic] = zero4;
            }
            const bool nt = vc & !triv;
            if (nt) Q[atomicAdd(cnt, 1)] = i;
            if constexpr (kTarget) {
                if (n > 0) {                 // st is row n - 1 of the history: its finished cotangent pair, for the sweep's owner of the cell
                    float ar, ay;
                    fit_pair(st.x, st.y, st.z, t_r, t_u, ar, ay);
                    if (vc) { float *tp = tp_run + ((int)ic - own0); tp[0] = ar; tp[N] = ay; }
                }
            }
        }
        if constexpr (kTarget) { tg_run += tail->gt_stride; tp_run += 2 * N; }
        lds_only_barrier();
        // ---- phase 2: the queued interfaces ----
        int k0 = tid - (rot << 6);
        if (k0 < 0) k0 += ncell;
        const unsigned i_q = (unsigned)Q[k0 <= N ? k0 : 0];
        const int qn = *cnt;
        if (k0 < qn) __builtin_amdgcn_s_setprio(3);
        for (int k = k0; k < qn; k += ncell) {
            const unsigned i = (k == k0) ? i_q : (unsigned)Q[k];
            const CellRec *lf = CR + i, *rt = CR + i + 1;
            const float4 ls = lf->st, rs = rt->st;
            const double2 lsh = lf->sh, lq0 = lf->q0, rsh = rt->sh;
            CellPre cl, cr;
            cl.s = lsh.x; cl.h = lsh.y; cl.q0 = lq0.x;
            cr.s = rsh.x; cr.h = rsh.y; cr.q0 = 0.;
            Iface f;
            arz_interface_fast_pre((double)ls.x, (double)ls.y, (double)ls.z, (double)ls.w, cl,
                                   (double)rs.x, (double)rs.y, (double)rs.z, (double)rs.w, cr, kc, f);
            FX[i] = make_double2(f.Fr, f.Fy);
            RA[i] = make_float4(f.A[0], f.A[1], f.A[2], f.A[3]);
            RB[i] = make_float4(f.B[0], f.B[1], f.B[2], f.B[3]);
        }
        __builtin_amdgcn_s_setprio(0);
        if (tid == 0) CNT[(n + 1) & 1] = 1;
        if (++rot == Wc) rot = 0;
        lds_only_barrier();
    };
    using yes = std::integral_constant<bool, true>;
    using no = std::integral_constant<bool, false>;

    const int C = (T + Sg - 1) / Sg;
    const float2 *ckp[2];                            // this thread's cells in the row that is loaded next (running pointers)
    // segment 0 starts from the call's inputs: loaded once, here, so that their four pointers are not carried through the loop
    float4 st0[2];
    float2 ck[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int i = lo + (j << 6) + t;                 // pass j < p of this thread (the plan names p = 1 or 2)
        const unsigned ic = (unsigned)(j < p && i < N ? i : N - 1);
        st0[j] = make_float4(r_in[base + ic], y_in[base + ic], u_in[base + ic], q_in[base + ic]);
        ckp[j] = ckpt + (size_t)(C > 1 ? C - 1 : 0) * ((size_t)L * N) + base + ic;
        ck[j] = C > 1 ? *ckp[j] : make_float2(0.f, 0.f);
    }
    if (kBound == kBoundConst && tid < 2) {          // constant boundary cells: their records once
        const float *g = ghost + (size_t)lane * 8 + (tid ? 4 : 0);
        const float4 st = make_float4(g[0], g[1], g[2], g[3]);
        CellPre cg;
        arz_cell_pre((double)st.x, um, cg);
        CellRec *gr = CR + (tid ? N + 1 : 0);
        gr->st = st; gr->sh = make_double2(cg.s, cg.h); gr->q0 = make_double2(cg.q0, 0.);
    }
    // kTarget: the row in front of the last segment's first step; the replay moves the pointer a row per step, and behind it the pointer
    // goes back to the row in front of the segment before (for segment 0 that is no row, and nothing is read there)
    if constexpr (kTarget) tg_run = target + (size_t)lane * 2 * N + own0 + ((ptrdiff_t)(C - 1) * Sg - 1) * ((ptrdiff_t)L * 2 * N);
    for (int seg = C - 1; seg >= 0; --seg) {
        const int s0 = seg * Sg, s1 = (T - s0 < Sg) ? T : s0 + Sg;
        // ---- the records step s0 starts from ----
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            int i = lo + (j << 6) + t, pj = p;
            // (kTarget: opaque, so that the masks below are formed here, once per segment, and hold no scalar registers across the
            // replay and the sweep, where this form has none to spare)
            if constexpr (kTarget) asm volatile("" : "+v"(i), "+v"(pj));
            const bool vc = j < pj && i < N;
            const unsigned ic = (unsigned)(vc ? i : N - 1);
            float4 st;
            CellPre cp;
            if (seg > 0) {
                st.x = ck[j].x; st.y = ck[j].y;
                cell_glue_pre(st.x, st.y, umf, kc, st.z, st.w, cp);
                if (seg > 1) { ckp[j] -= tail->ck_stride; ck[j] = *ckp[j]; }      // the row before: in flight across the whole segment
            } else {
                st = st0[j];
                arz_cell_pre((double)st.x, um, cp);
            }
            if (vc) {
                CellRec *own = CR + ic + 1;
                own->st = st; own->sh = make_double2(cp.s, cp.h);
                if constexpr (kRamp) own->q0.x = cp.q0; else own->q0 = make_double2(cp.q0, 0.);
            }
            if constexpr (kRing) ring_rec_copies<kRamp>(CR, Nv, vc, ic, st, cp);
            if constexpr (kRamp) {                       // row s0, for the update in the call of step s0 + 1: a whole step ahead
                const int rc = vc ? ramp_col_get(CR, ic) : 0;
                if (rc) { const float nx = rin[(size_t)s0 * L * n_ramp + (rc - 1)]; if (j) src1 = nx; else src0 = nx; }
            }
        }
        if constexpr (kSched) sched_p = sched_lane + (size_t)s0 * L * 2;
        if (kSched && tid < 2) {                         // a schedule: row s0
            const float4 st = *sched_p;
            CellPre cg;
            arz_cell_pre((double)st.x, um, cg);
            CellRec *gr = CR + (tid ? N + 1 : 0);
            gr->st = st; gr->sh = make_double2(cg.s, cg.h); gr->q0 = make_double2(cg.q0, 0.);
        }
        if constexpr (kSched) {
            sched_p += (size_t)L * 2;
            if (tid < 2 && s0 + 1 < s1) sched_st = *sched_p;
        }
        if (tid == 0) { Q[0] = N; CNT[0] = 1; CNT[1] = 1; }      // entry 0 of every step's queue: interface N
        if constexpr (kTarget) tp_run = tp0;
        lds_only_barrier();
        // ---- replay steps [s0, s1) into the ring ----
        body(no{}, s0, s1, R, R + (N + 1));
        for (int n = s0 + 1; n < s1; ++n) {
            float4 *RA = R + (size_t)(n - s0) * 2 * (N + 1);
            body(yes{}, n, s1, RA, RA + (N + 1));
        }
        if constexpr (kTarget) tg_run -= (ptrdiff_t)(s1 - s0 + Sg) * tail->gt_stride;
        // ---- sweep them newest first, out of the ring: macro_rollout_bwd_kernel's step ----
        for (int step = s1 - 1; step >= s0; --step) {
            const float4 *RA = R + (size_t)(step - s0) * 2 * (N + 1), *RB = RA + (N + 1);
            // kTaps: the columns that go in front of step - 1, loaded here and added behind the hand-over below
            float ar[2], ay[2];
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                ar[m] = 0.f; ay[m] = 0.f;
                if (kTaps && step > 0) {
                    gtp[m] -= tail->gt_stride;
                    if (col[m] >= 0) { ar[m] = gtp[m][0]; ay[m] = gtp[m][n_det]; }
                }
            }
            for (int k = tid; k < N; k += B) {
                float4 d0, d1, d2;
                const float4 aL = RA[k], bL = RB[k], aR = RA[k + 1], bR = RB[k + 1];
                cell_blocks(aL, bL, aR, bR, cf, ncf, d0, d1, d2);
                const float gr = Gr[k + 1], gy = Gy[k + 1];
                const float c0r = dot2(d0.x, gr, d0.z, gy), c0y = dot2(d0.y, gr, d0.w, gy);
                const float c1r = dot2(d1.x, gr, d1.z, gy), c1y = dot2(d1.y, gr, d1.w, gy);
                const float c2r = dot2(d2.x, gr, d2.z, gy), c2y = dot2(d2.y, gr, d2.w, gy);
                // c0 of cell k goes to cell k-1 (slot k), c2 of cell k goes to cell k+1 (slot k+2)
                C0r[k] = c0r; C0y[k] = c0y;
                C2r[k + 2] = c2r; C2y[k + 2] = c2y;
                Gr[k + 1] = c1r; Gy[k + 1] = c1y;
                // (a ring has no boundary cotangent: slot 0's goes to cell N - 1 and slot N + 1's to cell 0 in the hand-over below)
                if constexpr (kSched) {
                    if (k == 0) gs_run[0] = make_double2((double)c0r, (double)c0y);               // (thread 0: gs_run is the row's entry 0)
                    if (k == N - 1) gs_run[1 - (tid & 1)] = make_double2((double)c2r, (double)c2y);
                } else if constexpr (!kRing) {
                    if (k == 0) { ghl_r += (double)c0r; ghl_y += (double)c0y; }
                    if (k == N - 1) { ghr_r += (double)c2r; ghr_y += (double)c2y; }
                }
            }
            if constexpr (kSched) gs_run -= (ptrdiff_t)L * 2;
            lds_only_barrier();
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                const int k = tid + m * B;
                if (k < N) {
                    float c2lr, c2ly, c0rr, c0ry;
                    if constexpr (kRing) {           // the seam: c2 of cell N - 1 (slot N + 1) comes to cell 0, c0 of cell 0 (slot 0) to cell N - 1
                        const int kl = (k > 0) ? k + 1 : N + 1, kr = (k < N - 1) ? k + 1 : 0;
                        c2lr = C2r[kl]; c2ly = C2y[kl]; c0rr = C0r[kr]; c0ry = C0y[kr];
                    } else {
                        c2lr = (k > 0) ? C2r[k + 1] : 0.f; c2ly = (k > 0) ? C2y[k + 1] : 0.f;
                        c0rr = (k < N - 1) ? C0r[k + 1] : 0.f; c0ry = (k < N - 1) ? C0y[k + 1] : 0.f;
                    }
                    float nr = (Gr[k + 1] + c2lr) + c0rr;
                    float ny = (Gy[k + 1] + c2ly) + c0ry;
                    if (bad_step < 0 && !(isfinite(nr) && isfinite(ny))) { bad_step = step; bad_cell = k; }
                    if (kTaps && step > 0 && col[m] >= 0) { nr += ar[m]; ny += ay[m]; }      // in front of step - 1: Gr[det[j] + 1] += gt[j]
                    if constexpr (kTarget) {
                        if (step > 0) { const float *tp = tp0 + ((step - s0) * 2 * N + k - own0); nr += tp[0]; ny += tp[N]; }      // row step - 1
                    }
                    // kRamp: nr is now the cotangent of r in the state after step - 1, where that step's source went in
                    if constexpr (kRamp) {
                        const int rc = ramp_col_get(CR, (unsigned)k);
                        if (step > 0 && rc) gin[(size_t)(step - 1) * L * n_ramp + (rc - 1)] = (float)(dt * (double)nr);
                    }
                    Gr[k + 1] = nr; Gy[k + 1] = ny;
                }
            }
            lds_only_barrier();
        }
    }
    const BwdTail tl = *tail;                        // (read back: see BwdTail)
    for (int k = tid; k < N; k += B) { tl.g_r_out[k] = Gr[k + 1]; tl.g_y_out[k] = Gy[k + 1]; }
    if (kBound == kBoundConst && tl.g_ghost) {
        if (tid == 0) { tl.g_ghost[0] = ghl_r; tl.g_ghost[1] = ghl_y; }
        if (tid == (N - 1) % B) { tl.g_ghost[2] = ghr_r; tl.g_ghost[3] = ghr_y; }
    }
    if (bad_step >= 0) raise_fault(tl.err, DHTS_FAULT_NAN, bad_step, lane, bad_cell);
}
