// macro_fwd_jvp.inc -- the ARZ rollout and kK tangent directions of it in ONE kernel, no tape; included by macro_kernels.hip inside
// namespace dhts, after macro_jvp.inc.
//
// Forward mode walks the steps in the forward's own order, so the interface products (A_i, B_i) of a step are on chip at the moment the
// tangent sweep wants them: where macro_rollout_fwd2_kernel stores a step's tape entry, this kernel keeps the same floats in LDS, and
// the owner of cell k applies the cell's blocks to its tangents while it finishes the step.  Neither the 17.3 B per cell-step of tape
// nor anything else of size [T] exists unless the caller asks for detector readings.
//
// Arithmetic: the two kernels' own.  The primal is the lane kernel's step, statement for statement (arz_cell_pre, cell_glue_pre,
// arz_is_trivial_fast, arz_trivial_fast, arz_interface_fast_pre); a trivial interface leaves tape_trivial_A(TapeFp{fp[0], fp[2], fp[3]})
// and a zero B, a queued one its (f.A, f.B); cell k forms cell_blocks of the products of interfaces k and k + 1 and calls jvp_cell
// (macro_jvp.inc) per direction.  Nothing is restated: the primal outputs are dhts_macro_rollout_fwd's bits (lane or pair kernel: the
// two are bit-equal) and the tangents dhts_macro_rollout_jvp's (tests/test_macro_fwd_jvp_gpu.py).
//
// WHERE THE TANGENT STEP SITS: in the "finish the previous step" half of phase 1, beside the Godunov update.  There the owner of cell k
// reads FX[k] and FX[k + 1] of step n - 1 before the same phase overwrites FX[k] for step n; the products PA / PB are read in the same
// place and written where the fluxes are written (phase 1 for a trivial interface, phase 2 for a queued one), so the in-order argument
// that protects FX protects them: the only other reader of entry k + 1 is the thread to the right in the same wavefront (the same
// instruction, load before store), the same thread's next pass (later in program order) or another wavefront's first cell, whose
// interface is always queued (written behind the barrier).  The neighbours' tangents come from TN copies that alternate with the step
// parity, as in macro_rollout_jvp_kernel: step s reads copy s & 1 and writes the other one.  NO barrier is added to the lane kernel's two.
// Boundary tangents sit in slots 0 and N + 1 of the copy a step reads: a constant one (ghost_mode 1) goes into both copies once; of a
// schedule (ghost_mode 2) row n + 1 is stored in phase 2 of step n -- behind the barrier that ends the last read of that copy's slots,
// two barriers ahead of the next one -- out of a register that was loaded one step earlier.
//
// Layout of a launch: as macro_rollout_jvp_kernel's -- directions [0, n_act) of the pointers it is handed, a slot d >= n_act carries
// zeros and touches no memory.  Every launch of a call recomputes the primal and writes the same r_out .. q_out; the host hands taps and
// the forward's fault record to the first launch only (taps == NULL: the primal readings are not stored).  T >= 1 (the entry point
// copies for T = 0).
// Dynamic LDS: the lane kernel's records (CellRec [N + 2] | flux double2 [N + 1] | queue int [N + 2] | 2 counters, rounded up to 16 B)
//   | float4 PA [N + 1], PB [N + 1] | float2 TN [2 copies][kK][N + 2]   (index k + 1 of a copy = cell k)
// kBoundRing (a closed lane, DESIGN 4l): behind its own record the owner of cell N - 1 writes the same record to slot 0 and the owner
// of cell 0 to slot N + 1 -- the copies that interfaces 0 and N are solved from in phase 2, behind the barrier.  No thread reads slot
// N + 1 in phase 1; slot 0 is read there by thread 0 alone, whose interface is queued whatever it finds.
// Nv: the lane length in a VECTOR register (ring_len): the two slots are addressed from the thread's own one, N records below resp.
// above it, so that the seam holds no scalar register across the step loop, where these kernels have none to spare.
__device__ __forceinline__ int ring_len(int N) {
    int Nv = N;
    asm volatile("" : "+v"(Nv));
    return Nv;
}
// One test per pass (ring_seam) covers both copies: an end cell that owns one of them only (N > 1) writes its own slot again in the
// other's place (ring_lo / ring_hi = 0), the same bits it has just stored there.
__device__ __forceinline__ bool ring_seam(int Nv, bool vc, unsigned ic) { return vc && (ic == 0u || (int)ic == Nv - 1); }
__device__ __forceinline__ int ring_lo(int Nv, unsigned ic) { return (int)ic == Nv - 1 ? -Nv : 0; }       // slot 0 from cell N - 1's own
__device__ __forceinline__ int ring_hi(int Nv, unsigned ic) { return ic == 0u ? Nv : 0; }                 // slot N + 1 from cell 0's own
// kKeepPad: the second half of q0, which no step reads, is left as it is (the checkpointed reverse kernel's ramp forms keep a cell's
// ramp column there, macro_ckpt.inc)
template <bool kKeepPad = false>
__device__ __forceinline__ void ring_rec_copies(CellRec *CR, int Nv, bool vc, unsigned ic, const float4 &st, const CellPre &cp) {
    if (ring_seam(Nv, vc, ic)) {
        CellRec *own = CR + ic + 1, *w = own + ring_lo(Nv, ic);
        w->st = st; w->sh = make_double2(cp.s, cp.h);
        if constexpr (kKeepPad) w->q0.x = cp.q0; else w->q0 = make_double2(cp.q0, 0.);
        w = own + ring_hi(Nv, ic);
        w->st = st; w->sh = make_double2(cp.s, cp.h);
        if constexpr (kKeepPad) w->q0.x = cp.q0; else w->q0 = make_double2(cp.q0, 0.);
    }
}
// ... and where scalar registers are to spare (the checkpointed forward): the two slots at their own addresses, a test each
__device__ __forceinline__ void ring_rec_copies_direct(CellRec *CR, int N, bool vc, unsigned ic, const float4 &st, const CellPre &cp) {
    if (vc && ic == (unsigned)(N - 1)) { CR[0].st = st; CR[0].sh = make_double2(cp.s, cp.h); CR[0].q0 = make_double2(cp.q0, 0.); }
    if (vc && ic == 0u) { CR[N + 1].st = st; CR[N + 1].sh = make_double2(cp.s, cp.h); CR[N + 1].q0 = make_double2(cp.q0, 0.); }
}
// kRamp (the kernel's last template argument; dhts_macro_rollout_fwd_jvp_ramp / _ring_ramp, DESIGN 4n): DESIGN 4m's source in chosen cells and
// its tangent.  A ramp cell finds its column of ramps[] + 1 in the second half of its record's q0 (ramp_col_set / ramp_col_get,
// macro_ckpt.inc: declared here, defined there), which the ramp forms leave as it is.
__device__ __forceinline__ void ramp_col_set(CellRec *CR, unsigned cell, int col1);
__device__ __forceinline__ int ramp_col_get(const CellRec *CR, unsigned cell);
// the loads that fill ts have all been issued and have arrived behind this line: none of them is moved down to its use, where each
// would wait for its own round trip in turn
template <int kK>
__device__ __forceinline__ void ramp_arrived(float (&ts)[kK]) {
    static_assert(kK == 1 || kK == 2 || kK == 4, "one operand per direction");
    if constexpr (kK == 1) asm volatile("" : "+v"(ts[0]));
    else if constexpr (kK == 2) asm volatile("" : "+v"(ts[0]), "+v"(ts[1]));
    else asm volatile("" : "+v"(ts[0]), "+v"(ts[1]), "+v"(ts[2]), "+v"(ts[3]));
}
__host__ __device__ inline size_t fwd_jvp_rec_bytes(int N) {       // = fwd2_lds_bytes(N) rounded up to 16
    return (sizeof(CellRec) * (size_t)(N + 2) + 16 * (size_t)(N + 1) + sizeof(int) * (size_t)(N + 2) + 16 + 15) & ~(size_t)15;
}
__host__ __device__ inline size_t fwd_jvp_lds_bytes(int N, int kK) {
    return fwd_jvp_rec_bytes(N) + 2 * 16 * (size_t)(N + 1) + 2 * 8 * (size_t)kK * (size_t)(N + 2);
}

// grid = L workgroups (one traffic lane each) of W = blockDim.x / 64 wavefronts, the lane kernel's mapping: wave w owns the cells
// [64 p w, 64 p (w + 1)), thread t of its pass j the cell 64 p w + 64 j + t and that cell's LEFT interface.  kP: 64-cell passes per
// wavefront as a literal (1 or 2; 0 = the run-time value p_arg), kBound: constant boundary cells, a schedule (kSched) or a ring (kRing),
// kSched / kTaps as in macro_rollout_fwd2_kernel (validity masks are
// always on: the lane kernel's kFull saves a few selects and changes no value).  At most 12 wavefronts: the longest lane whose LDS fits
// (1410 cells) has 12, and three wavefronts per SIMD leave the kernel 168 VGPRs -- two interleaved passes beside four directions
// spill under the 128 of a 1024-thread block.
// err: DHTS_FAULT_CFL (step, lane, interface), as the lane kernel raises it.  err_jvp: DHTS_FAULT_NAN with the lane's EARLIEST
// (step, cell) of a non-finite tangent (jvp_raise_first).
// kRamp: ramps [n_ramp] cell indices shared by all lanes, inflow [T][L][n_ramp], t_inflow [kK][T][L][n_ramp] or NULL (zero tangents).  Behind
// the Godunov update of step s the owner of cell ramps[j] forms r' = (float)((double)r + dt (double)inflow[s][l][j]) and, behind jvp_cell,
// nr' = (float)((double)nr + dt (double)t_inflow[d][s][l][j]) for d < n_act; y and ny stay.  Both additions are in front of everything that
// reads the state or the tangents after step s: the record, the kept rd_own, the copy the next step reads, the ring's seam copies, the
// finiteness test, the outputs and the readings.  With kP = 1 or 2 the owner holds its 1 + kK entries of the row its next update adds
// in registers, asked for a whole step ahead (ramp_src / ramp_tan below): no global load is on any wavefront's dependent chain.  With a
// run-time number of passes it loads them in the step, all at once (ramp_arrived); a wavefront without a ramp cell branches round the
// loads (its threads find column 0 in their records), so none of them is on its chain.
// Thread q writes column q + 1 into the record of cell ramps[q] once, behind the prologue's barrier; the first reader is behind one more
// barrier of the prologue (kP = 1, 2) resp. the update of step 0, two barriers later.  An entry of ramps outside [0, N) is compared as
// an unsigned value and forms no address.  No barrier is added to the step loop, no atomic and no LDS anywhere; with kRamp false the
// kernel is the one it was.
template <int kK, int kP, MacroBoundary kBound, bool kTaps, bool kRamp>
__global__ __launch_bounds__(768) void macro_rollout_fwd_jvp_kernel(
    int L, int N, int T, int p_arg, double dt, double dx, double um,
    const float *__restrict__ r_in, const float *__restrict__ y_in, const float *__restrict__ u_in,
    const float *__restrict__ q_in, const float *__restrict__ ghost,
    const float *__restrict__ t_r_in, const float *__restrict__ t_y_in, const float *__restrict__ t_ghost, int ghost_mode, int n_act,
    float *__restrict__ r_out, float *__restrict__ y_out, float *__restrict__ u_out, float *__restrict__ q_out,
    float *__restrict__ t_r_out, float *__restrict__ t_y_out,
    const int32_t *__restrict__ det, int n_det, float *__restrict__ taps, float *__restrict__ t_taps,
    dhts_error *err, dhts_error *err_jvp,
    const int32_t *__restrict__ ramps, int n_ramp, const float *__restrict__ inflow, const float *__restrict__ t_inflow) {
    constexpr bool kSched = kBound == kBoundSched, kRing = kBound == kBoundRing;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = blockIdx.x;
    const int tid = threadIdx.x;
    const int t = tid & 63;
    const int wv = tid >> 6;
    const int Wc = blockDim.x >> 6;                  // wavefronts
    const int ncell = blockDim.x;
    const int P = N + 2;
    const size_t base = (size_t)lane * N;
    CellRec *CR = reinterpret_cast<CellRec *>(smem);
    double2 *FX = reinterpret_cast<double2 *>(CR + (N + 2));
    int *Q = reinterpret_cast<int *>(FX + (N + 1));
    int *CNT = Q + (N + 2);                          // queue length by step parity
    float4 *PA = reinterpret_cast<float4 *>(smem + fwd_jvp_rec_bytes(N)), *PB = PA + (N + 1);      // products of interface i
    float2 *TN = reinterpret_cast<float2 *>(PB + (N + 1));                                         // [copy][kK][P]
    IfaceConst kc;
    kc.set_um(um); kc.set_grid(dt, dx);
    const size_t dir_state = (size_t)L * N;
    const size_t dir_ghost = (ghost_mode == 2 ? (size_t)T : 1) * L * 4;
    const size_t dir_taps = (size_t)T * L * 2 * n_det;

    for (int k = tid; k < N + 2; k += blockDim.x) {
        float4 st;
        if (!kRing && (k == 0 || k == N + 1)) {
            const float *g = ghost + (size_t)lane * 8 + (k ? 4 : 0);
            st = make_float4(g[0], g[1], g[2], g[3]);
        } else {
            const int kc_ = kRing ? (k == 0 ? N : (k == N + 1 ? 1 : k)) : k;      // a ring: slot 0 is cell N - 1, slot N + 1 is cell 0
            st = make_float4(r_in[base + kc_ - 1], y_in[base + kc_ - 1], u_in[base + kc_ - 1], q_in[base + kc_ - 1]);
        }
        CellPre c;
        arz_cell_pre((double)st.x, um, c);
        CR[k].st = st;
        CR[k].sh = make_double2(c.s, c.h);
        CR[k].q0 = make_double2(c.q0, 0.);
    }
    for (int i = tid; i < 2 * kK * P; i += blockDim.x) TN[i] = make_float2(0.f, 0.f);
    if (tid == 0) { Q[0] = N; CNT[0] = 1; CNT[1] = 1; }      // entry 0 of every step's queue: interface N
    __syncthreads();
    if constexpr (kRamp) {
        for (int q = tid; q < n_ramp; q += blockDim.x) {
            const unsigned rc = (unsigned)ramps[q];
            if (rc < (unsigned)N) ramp_col_set(CR, rc, q + 1);
        }
    }
    // the tangents of the initial state into copy 0
    for (int d = 0; d < n_act; ++d)
        for (int k = tid; k < N; k += blockDim.x) {
            const float2 v = make_float2(t_r_in[d * dir_state + base + k], t_y_in[d * dir_state + base + k]);
            TN[d * P + k + 1] = v;
            if constexpr (kRing) {
                if (k == N - 1) TN[d * P] = v;
                if (k == 0) TN[d * P + N + 1] = v;
            }
        }

    const int p = kP > 0 ? kP : p_arg;
    const int lo = wv * (p << 6);                    // first cell of this wave
    const double c = dt / dx;                        // update_coefficient, _macro_lane.py:99
    const float cf = (float)c, ncf = (float)(-c);
    const float umf = (float)um;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    int fault_step = -1, fault_index = 0;
    int bad_step = -1, bad_cell = 0;
    int rot = 0;                                     // the cell wave that takes the head of the queue rotates with the step

    const int Nv = kRing && kTaps ? ring_len(N) : N; // (a ring with detectors, where no scalar register is to spare: see ring_rec_copies)
    constexpr bool kKeep = kP > 0;
    double rd_own[kP > 0 ? kP : 1], yd_own[kP > 0 ? kP : 1];
    // kRamp with a literal number of passes (kPre): the entries of inflow and t_inflow that the thread's next update adds wait in
    // registers, one row per pass, asked for a whole step ahead as the checkpointed forward does -- no global load on the step's
    // dependent chain at all.  A run-time number of passes (kP = 0, DHTS_OPT_MACRO_FWD_WAVES alone) would index them at run time, which is
    // scratch: there the owner loads in the step.  ramp_load: the 1 + n_act entries of row `row` for column rc (t_inflow NULL or a slot
    // d >= n_act: 0, nothing is read).
    constexpr bool kPre = kRamp && kP > 0;
    const size_t dir_inflow = kRamp ? (size_t)T * L * n_ramp : 0;
    float ramp_src[kP > 0 ? kP : 1], ramp_tan[kP > 0 ? kP : 1][kK];
    auto ramp_load = [&](const int row, const int rc, float &s, float (&ts)[kK]) {
        const size_t e = ((size_t)row * L + lane) * n_ramp + (rc - 1);
        s = inflow[e];
#pragma unroll
        for (int d = 0; d < kK; ++d) ts[d] = t_inflow && d < n_act ? t_inflow[d * dir_inflow + e] : 0.f;
    };
    if constexpr (kPre) {
        __syncthreads();                             // the columns are in the records (once per launch: the step loop takes no barrier more)
#pragma unroll
        for (int j = 0; j < kP; ++j) {
            const int i = lo + (j << 6) + t;
            const int rc = i < N ? ramp_col_get(CR, (unsigned)i) : 0;
            ramp_src[j] = 0.f;
#pragma unroll
            for (int d = 0; d < kK; ++d) ramp_tan[j][d] = 0.f;
            if (rc) ramp_load(0, rc, ramp_src[j], ramp_tan[j]);
        }
    }

    float4 sched_st = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 *sched_p = nullptr;
    if constexpr (kSched) {
        sched_p = reinterpret_cast<const float4 *>(ghost) + ((size_t)L + lane) * 2 + (tid & 1);
        if (tid < 2 && T > 1) sched_st = *sched_p;
    }
    // the LAST threads of the lane read for the others: thread (blockDim - 1 - tid) = tap_j takes detector slot tap_j (+ blockDim per
    // further one) and, for tap_j < 2 kK, the boundary tangent (direction tap_j >> 1, side tap_j & 1)
    const int tap_j = (int)blockDim.x - 1 - tid;
    int det_own = -1;
    bool tap_wave = false;
    if constexpr (kTaps) {
        tap_wave = __builtin_amdgcn_readfirstlane((Wc - 1 - wv) << 6) < n_det;
        if (tap_j < n_det) det_own = det[tap_j];
    }
    const bool bnd = !kRing && ghost_mode != 0 && tap_j < 2 * kK && (tap_j >> 1) < n_act;       // (a ring has no boundary tangent)
    const int bnd_slot = (tap_j >> 1) * P + ((tap_j & 1) ? N + 1 : 0);
    const float *bnd_src = bnd ? t_ghost + (size_t)(tap_j >> 1) * dir_ghost + (size_t)lane * 4 + 2 * (tap_j & 1) : nullptr;
    const size_t bnd_stride = (size_t)L * 4;
    float2 bnd_next = make_float2(0.f, 0.f);         // a schedule: row n + 1, one step ahead of its store
    if (bnd) {
        const float2 v = *reinterpret_cast<const float2 *>(bnd_src);          // row 0, or the constant tangent
        TN[bnd_slot] = v;
        if (ghost_mode == 1) TN[kK * P + bnd_slot] = v;
        else if (T > 1) bnd_next = *reinterpret_cast<const float2 *>(bnd_src + bnd_stride);
    }
    auto tap = [&](const int s) {                       // the state and the tangents after step s: the records, the copy step s wrote
        if (tap_wave) {
            const CellRec *cr = CR;
            if (taps)
                taps_write(det, n_det, det_own, tap_j, (int)blockDim.x, N, taps + ((size_t)s * L + lane) * 3 * n_det,
                           [=](unsigned dc) { return cr[dc + 1].st; });
            const float2 *tw = TN + ((s & 1) ^ 1) * kK * P;
            float *row = t_taps + ((size_t)s * L + lane) * 2 * n_det;
            for (int j = tap_j; j < n_det; j += (int)blockDim.x) {
                const unsigned dc = (unsigned)(j == tap_j ? det_own : det[j]);
                if (dc < (unsigned)N) {
#pragma unroll
                    for (int d = 0; d < kK; ++d) {
                        if (d < n_act) {
                            const float2 v = tw[d * P + dc + 1];
                            row[d * dir_taps + j] = v.x; row[d * dir_taps + n_det + j] = v.y;
                        }
                    }
                }
            }
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
        int *cnt = CNT + (n & 1);
        const float2 *tq = TN + ((n - 1) & 1) * kK * P;    // the copy step n - 1 reads ...
        float2 *tw = TN + (n & 1) * kK * P;                // ... and the one it writes
#pragma unroll
        for (int j = 0; j < p; ++j) {
            const int i = lo + (j << 6) + t;                // cell i and its left interface i
            const bool vc = i < N;
            const unsigned ic = (unsigned)(vc ? i : N - 1);
            CellRec *own = CR + ic + 1;
            float4 st;
            if (!(kKeep && upd)) st = own->st;
            if (kKeep && !upd) { rd_own[kP > 0 ? j : 0] = (double)st.x; yd_own[kP > 0 ? j : 0] = (double)st.y; }
            if (upd) {
                // Godunov update, _macro_lane.py:109-112, float32 store :327-334
                const double2 Fl = FX[ic], Fr = FX[ic + 1];
                // the tangents of step n - 1 (dmacro_lane.py:126-129 applied untransposed): the products of the cell's two interfaces,
                // read where the fluxes are read
                const float4 aL = PA[ic], bL = PB[ic], aR = PA[ic + 1], bR = PB[ic + 1];
                int rc = 0;                                  // kRamp: the cell's column of ramps[] + 1, read beside the products
                if constexpr (kRamp) rc = vc ? ramp_col_get(CR, ic) : 0;
                JvpBlocks b;
                cell_blocks(aL, bL, aR, bR, cf, ncf, b.d0, b.d1, b.d2);
                bool fin = true;
                const bool seam = kRing && ring_seam(Nv, vc, ic);
#pragma unroll
                for (int d = 0; d < kK; ++d) {
                    const float2 tl = tq[d * P + ic], tc = tq[d * P + ic + 1], tr = tq[d * P + ic + 2];
                    float nr, ny;
                    jvp_cell(b, tl.x, tl.y, tc.x, tc.y, tr.x, tr.y, nr, ny);
                    if constexpr (kPre) {                    // the tangent of the on-ramp's source of step n - 1 (a slot d >= n_act holds 0)
                        if (rc && t_inflow) nr = (float)((double)nr + dt * (double)ramp_tan[kP > 0 ? j : 0][d]);
                    }
                    if (vc) tw[d * P + ic + 1] = make_float2(nr, ny);
                    if constexpr (kRing) {                   // the copy step n reads: slot 0 is cell N - 1, slot N + 1 is cell 0
                        if (seam) {
                            float2 *own_t = tw + d * P + ic + 1;
                            own_t[ring_lo(Nv, ic)] = make_float2(nr, ny); own_t[ring_hi(Nv, ic)] = make_float2(nr, ny);
                        }
                    }
                    fin = fin && isfinite(nr) && isfinite(ny);
                    if (!solve && vc && d < n_act) { t_r_out[d * dir_state + base + i] = nr; t_y_out[d * dir_state + base + i] = ny; }
                }
                float src = 0.f;
                if constexpr (kPre) {
                    // the source of step n - 1 is in the register; row n leaves for it, a whole step ahead of the update that adds it
                    src = ramp_src[kP > 0 ? j : 0];
                    if (rc && solve) ramp_load(n, rc, ramp_src[kP > 0 ? j : 0], ramp_tan[kP > 0 ? j : 0]);
                }
                if constexpr (kRamp && !kPre) {
                    // a run-time number of passes holds no row in registers: the owner asks for its 1 + n_act entries of row n - 1 here, all
                    // of them before it waits for the first, and adds the tangents to what it has just stored, in front of every reader
                    if (rc) {
                        float ts[kK];
                        ramp_load(n - 1, rc, src, ts);
                        ramp_arrived(ts);
                        if (t_inflow) {
#pragma unroll
                            for (int d = 0; d < kK; ++d) {
                                if (d < n_act) {
                                    float2 *own_t = tw + d * P + ic + 1;
                                    float2 v = *own_t;
                                    v.x = (float)((double)v.x + dt * (double)ts[d]);
                                    *own_t = v;
                                    if constexpr (kRing) {
                                        if (seam) { own_t[ring_lo(Nv, ic)] = v; own_t[ring_hi(Nv, ic)] = v; }
                                    }
                                    fin = fin && isfinite(v.x);
                                    if (!solve) t_r_out[d * dir_state + base + i] = v.x;
                                }
                            }
                        }
                    }
                }
                if (vc && bad_step < 0 && !fin) { bad_step = n - 1; bad_cell = i; }
                const double r_old = kKeep ? rd_own[kP > 0 ? j : 0] : (double)st.x;
                const double y_old = kKeep ? yd_own[kP > 0 ? j : 0] : (double)st.y;
                st.x = (float)(r_old + (Fl.x - Fr.x) * c);
                st.y = (float)(y_old + (Fl.y - Fr.y) * c);
                if constexpr (kRamp) {
                    if (rc) st.x = (float)((double)st.x + dt * (double)src);
                }
                if (kKeep) { rd_own[kP > 0 ? j : 0] = (double)st.x; yd_own[kP > 0 ? j : 0] = (double)st.y; }
                CellPre cp;
                cell_glue_pre(st.x, st.y, umf, kc, st.z, st.w, cp);     // set_next_state_vector_y, :282-299
                if (vc && solve) {
                    own->st = st; own->sh = make_double2(cp.s, cp.h);
                    if constexpr (kRamp) own->q0.x = cp.q0; else own->q0 = make_double2(cp.q0, 0.);
                }
                else if (kTaps && vc) own->st = st;          // the final step's state, for the taps below
                if constexpr (kRing && solve) ring_rec_copies<kRamp>(CR, Nv, vc, ic, st, cp);
            }
            if (!solve) {
                if (vc) { r_out[base + i] = st.x; y_out[base + i] = st.y; u_out[base + i] = st.z; q_out[base + i] = st.w; }
                continue;
            }
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
            if (triv) {
                FX[ic] = make_double2(Fr, Fy);
                PA[ic] = tape_trivial_A(TapeFp{fp[0], fp[2], fp[3]});      // what the lane kernel's tape entry expands to
                PB[ic] = zero4;
            }
            const bool nt = vc & !triv;
            if (nt) Q[atomicAdd(cnt, 1)] = i;
        }
        if (!solve) {
            if constexpr (kTaps && upd) { lds_only_barrier(); tap(n - 1); }
            return;
        }
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
            PA[i] = make_float4(f.A[0], f.A[1], f.A[2], f.A[3]);
            PB[i] = make_float4(f.B[0], f.B[1], f.B[2], f.B[3]);
            if (f.cfl_bad && fault_step < 0) { fault_step = n; fault_index = (kRing && i == (unsigned)N) ? 0 : (int)i; }      // (a ring: N is 0)
        }
        __builtin_amdgcn_s_setprio(0);
        if constexpr (kTaps && upd) tap(n - 1);
        if (!kRing && ghost_mode == 2 && bnd && n + 1 < T) {           // row n + 1 into the copy step n + 1 reads
            TN[((n + 1) & 1) * kK * P + bnd_slot] = bnd_next;
            if (n + 2 < T) bnd_next = *reinterpret_cast<const float2 *>(bnd_src + (size_t)(n + 2) * bnd_stride);
        }
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
    jvp_raise_first(reinterpret_cast<unsigned *>(CNT), bad_step, bad_cell, lane, err_jvp);
}
