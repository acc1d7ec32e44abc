// macro_fwd_pairs.inc -- the two-phase rollout forward kernel with a thread owning two ADJACENT cells and their RIGHT interfaces
// (included by macro_kernels.hip inside namespace dhts; what dhts_macro_rollout_fwd launches for full lanes of 128 W cells).
//
// The lane / lane-group kernels above hand a cell's 48-byte record to its right neighbour's thread through LDS (three 16-byte
// stores, three 16-byte loads, a store -> load round trip in the middle of every pass) and that thread widens the neighbour's
// float32 state again and redoes what the owner had in registers: max(r, eps), 1 / r, u_eq'(r), y / r.  But everything the
// trivial solve of an interface needs is a function of its LEFT cell alone (Q_0 = Q_L: flux, flux Jacobian, lambda_0(Q_L)); of
// the right cell only "is it vacuum" and its speed enter the classification (arz_is_trivial_fast).  So here
//   * thread m of a traffic lane owns cells 2m and 2m + 1 for the whole rollout (their (r, y) stay in registers as doubles) and
//     the interfaces 2m + 1 (between its own cells: nothing to fetch) and 2m + 2 (right cell = thread m + 1's first cell: its
//     float32 speed arrives by ONE DPP wave shift, its vacuum / CFL flags as the wavefront's lane masks shifted by one);
//   * the last interface of a wavefront's chunk (128 (w + 1): its right cell belongs to another wavefront or is the right ghost)
//     and interface 0 (no owner) are STANDING entries 0 .. W of the lane's queue, written once;
//   * the cell records are still written (phase 2 reads both cells of a queued interface from them) but phase 1 never reads
//     them; fluxes and records lie split by parity (even | odd) so that a thread's two neighbouring entries are 16-byte
//     accesses at a 16- resp. 48-byte lane stride: no bank conflicts;
//   * a wavefront none of whose cells is (nearly) empty -- practically always on a road with traffic -- runs phase 1 without
//     the clamps and vacuum selects (own_glue<true>: same values, ~25 vector instructions per thread fewer);
//   * phase 2 is arz_interface_queued (case logic on lane masks, one branch-free stream) with a STATIC assignment: thread g takes
//     entry g / G of lane g % G's queue, so the queue entry and the count are read side by side (one LDS round trip less on
//     the serial path) and every tape address is a uniform row pointer + a 32-bit offset;
//   * the two workgroups of a CU: the one dispatched later loses the issue arbitration (age), falls behind and ends up running
//     alone; the workgroups of the second half of the grid therefore take turns with the others at priority 1, eight steps at a time.
// Every float32 / double operation is that of the lane kernel (macro_rollout_fwd2_kernel): final state and what the reverse sweep makes of the
// tape are bit-identical (tests/test_gpu_parity.py::test_macro_pair_kernel_equals_lane_kernel); the exception lists come in another order.
// Measured on BASELINE config 2 (MI355X, same box, profiles/r04*): lane-group kernel 3.15-3.30 ms, this kernel 2.62-2.70 ms.
//
// LDS per traffic lane (H = N / 2):
//   CellRec [N + 2]: slot k <= H: cell 2k (k = H: the right ghost = "cell N"); slot H + 1 + j: cell 2j - 1 (j = 0: the left ghost)
//   double2 FXe [H + 1]: flux of interface 2k | double2 FXo [H]: flux of interface 2k + 1 | int Q [N + 2] | int CNT [2] (+ pad)
__host__ __device__ inline size_t fwd3_region_bytes(int N) {
    const size_t H = (size_t)N / 2;
    return (sizeof(CellRec) * (size_t)(N + 2) + 16 * (H + 1) + 16 * H + sizeof(int) * (size_t)(N + 2) + 16 + 15) & ~(size_t)15;
}

// What a cell's owner knows about it after the float32 glue (cell_glue_pre, operation for operation) -- kept apart so that the
// interface to the cell's right can share max(r, eps), 1 / max(r, eps) and the float32 square root with it.
struct OwnPre {
    double rLc, s, h, q0;   // max(r, eps), its square root, 0.5 / that, u_eq(r) in double (CellPre)
    double inv;             // 1 / max(r, eps) = (2 h)^2
    float s32;              // float32(sqrt(max(r, 0) + eps)) as the glue forms it (>= sqrt(max(r, eps)) (1 - 1e-6) for r >= 0)
};
// kDense: the caller knows r > float32(eps) (hence r > eps in double, r > 0): every clamp and every vacuum select of the glue
// picks its ordinary operand -- the same values with a dozen instructions fewer.  A wavefront takes that form when none of its
// cells is (nearly) empty, i.e. practically always on a road with traffic; the general form is the fallback (wave-uniform branch).
template <bool kDense>
__device__ __forceinline__ void own_glue(float r, double rd, double yd, float umf, const IfaceConst &k, float &u, float &q, OwnPre &o) {
    o.rLc = kDense ? rd : fmax(rd, kEps);
    sqrt_hrsqrt(o.rLc, o.s, o.h);
    const double tE = (kDense ? rd : fmax(rd, 0.)) + kEps;
    double sE, hE;
    sqrt_hrsqrt(tE, sE, hE);
    o.q0 = __builtin_fma(-k.um, sE, k.um);
    const float t32 = r + kEpsF;
    o.s32 = (float)__builtin_fma((double)t32 - tE, hE, sE);
    const float one_m = 1.f - o.s32;
    q = (!kDense && 0.f > r) ? k.ueq_neg_f : umf * one_m;
    const double rs = o.h + o.h;
    o.inv = rs * rs;
    const double invg = (!kDense && r <= kEpsF) ? k.inv_epsf : o.inv;
    const float yor = (float)(yd * invg);
    u = yor + ((!kDense && r < kEpsF) ? k.ueq_2eps_f : q);
}
// the same for a state that was given (step 0): arz_cell_pre's values
__device__ __forceinline__ void own_pre_init(double rd, const IfaceConst &k, OwnPre &o) {
    o.rLc = fmax(rd, kEps);
    sqrt_hrsqrt(o.rLc, o.s, o.h);
    const double sE = fast_sqrt(fmax(rd, 0.) + kEps);
    o.q0 = __builtin_fma(-k.um, sE, k.um);
    const double rs = o.h + o.h;
    o.inv = rs * rs;
    o.s32 = (float)sE * 1.000001f;
}
// A cell's share of the bound on every speed the solver can report at the interfaces it touches (arz_is_trivial_fast):
// g = |u| + |u_eq| / 2 + u_max (1 + sqrt(r)) / 2 >= |u|.  If g < thr for both cells of an interface, the interface's bound
// |u_L| + |u_R| + |u_eq,L| / 2 + u_max (1 + sqrt(r_L)) / 2 <= g_L + g_R is inside the CFL limit; thr = (dx / dt) / 2 less the float32
// rounding (1e-4 relative) and what |s32| can miss of sqrt(max(r, eps)) for a negative density (sqrt(eps) u_max / 2).  A cell that
// fails sends its two interfaces to the full solver with its exact CFL test -- the results are the same either way.
// (the constant term u_max / 2 sits in the threshold)
__device__ __forceinline__ float own_calm_thr(const IfaceConst &k) {
    const double thr = 0.5 * k.cfl_lim * (1.0 - 1e-4) - 0.002 * k.um - 0.5 * k.um;
    return k.lim_ok ? (float)thr : -1.f;
}
// (two v_fma_f32 with |.| source modifiers, written out: left to itself the compiler pairs the two cells' operations into packed
// float32 instructions, which have no |.| modifier and need a v_and_b32 per operand first)
__device__ __forceinline__ bool own_calm(float u, float q, float s32, float half_um, float thr) {
    float g;
    asm("v_fma_f32 %0, 0.5, |%1|, |%2|" : "=v"(g) : "v"(q), "v"(u));
    asm("v_fma_f32 %0, %1, |%2|, %0" : "+v"(g) : "v"(half_um), "v"(s32));
    return g < thr;
}
// The trivial solve of the interface right of an own cell (arz_is_trivial_fast_v + arz_trivial_fast, operation for operation,
// with the left cell's quantities taken from OwnPre): is Q_0 = Q_L, its flux, its flux Jacobian.
// kDense: neither cell of the interface is (nearly) empty: vacL = vacR = 0 as literals.
// The case logic runs on LANE MASKS, as phase 2's does (arz_interface_queued): every compare feeds its own ballot and the booleans are
// combined as 64-bit scalars -- held as bools the compiler materialises them as 0 / 1 in vector registers and compares them again
// (five vector instructions per interface).  Called by whole wavefronts only (EXEC = all ones: ~mask needs no masking).
typedef unsigned long long LaneMask;
template <bool kDense>
__device__ __forceinline__ LaneMask own_iface(double rd, double yd, float u32, double ud, const OwnPre &o, LaneMask vacL_, LaneMask vacR_,
                                              float uR32, double uRd, const IfaceConst &k, double &Fr, double &Fy, TapeFp &fp) {
    const LaneMask vacL = kDense ? 0 : vacL_, vacR = kDense ? 0 : vacR_;
    const double ueqp = -k.um * o.h;
    const double dU = ud - uRd;
    const LaneMask same = __builtin_amdgcn_ballot_w64(fabs(dU) < kEps);
    const LaneMask b4 = ~(vacL | vacR | same) & __builtin_amdgcn_ballot_w64(u32 > uR32);
    const double bm = __builtin_fma(dU, k.inv_um, o.s);
    const double rm = bm * bm;
    const double l0l = __builtin_fma(rd, ueqp, ud);
    const double diff = __builtin_fma(rm, uRd, -(rd * ud));
    const LaneMask zero0 = vacL | (same & ~vacR);
    const LaneMask triv = zero0 | (b4 & __builtin_amdgcn_ballot_w64(diff >= 0.0)) | (~b4 & __builtin_amdgcn_ballot_w64(l0l >= 0.0));
    const double qc = (!kDense && __builtin_amdgcn_inverse_ballot_w64(vacL)) ? k.ueq_2eps : o.q0;
    const double u0 = __builtin_fma(yd, o.inv, qc);
    Fr = rd * u0;
    Fy = yd * u0;
    const double yor = yd * o.inv;
    fp.f0 = (float)__builtin_fma(o.rLc, ueqp, o.q0);
    fp.f2 = (float)__builtin_fma(yd, ueqp, -(yor * yor));
    fp.f3 = (float)__builtin_fma(yd + yd, o.inv, o.q0);
    return triv;
}

// Phase timing for tools/probes/exp_fwd3_stamps.py: compiled in with -DDHTS_FWD3_STAMPS only (a separate build of the library,
// never the product).  s_memtime around both barriers of a step, summed over the steps per wavefront of workgroups 0 .. 7 and
// G / 2 .. G / 2 + 7: [0] phase-1 work, [1] wait at barrier 1, [2] phase-2 work and [3] wait at barrier 2 in steps where the
// wavefront held queue entries ([6], [7]: in steps where it held none), [4] steps in which it held entries, [5] entries it solved.
#ifdef DHTS_FWD3_STAMPS
__device__ long long dhts_fwd3_stamps[16][16][8];
__device__ long long dhts_fwd_clock[2][16][2];      // [kernel: 0 = lane-group, 1 = pair][workgroup][s_memtime ticks, s_memrealtime ticks (100 MHz)] over the step loop
#define FWD3_STAMP(i) { const long long now_ = __builtin_amdgcn_s_memtime(); st_acc_[i] += now_ - st_last_; st_last_ = now_; }
#else
#define FWD3_STAMP(i)
#endif

// One thread's phase 1 behind the Godunov update: the float32 glue of its two cells (upd), their records for phase 2, and the
// trivial solves of its two right interfaces (solve).  kDense: see own_glue.
struct PairOut {
    double Fr1, Fy1, Fr2, Fy2;
    TapeFp fp1, fp2;
    LaneMask easy1, triv2;      // lane masks: interface 2m + 1 / 2m + 2 is trivial and inside the cheap CFL bound
};
template <bool kDense, bool kUpd, bool kSolve>
__device__ __forceinline__ void pair_phase1(float ra, float ya, float rb, float yb, double rda, double yda, double rdb, double ydb,
                                            float &ua, float &qa, float &ub, float &qb, OwnPre &A, OwnPre &B, CellRec *CRa, CellRec *CRb,
                                            float umf, float half_um, float calm_thr, const IfaceConst &kc, PairOut &o) {
    if (kUpd) {
        own_glue<kDense>(ra, rda, yda, umf, kc, ua, qa, A);
        own_glue<kDense>(rb, rdb, ydb, umf, kc, ub, qb, B);
        if (kSolve) {
            CRa->st = make_float4(ra, ya, ua, qa); CRa->sh = make_double2(A.s, A.h); CRa->q0.x = A.q0;
            CRb->st = make_float4(rb, yb, ub, qb); CRb->sh = make_double2(B.s, B.h); CRb->q0.x = B.q0;
        }
    }
    if (kSolve) {
        // of the cell right of this thread's second cell (the next thread's first): its speed by a DPP wave shift, its flags as the
        // wavefront's lane masks moved down by one (lane 63 gets nothing useful: that interface is queued)
        const float un = take_right(ua, ua);
        const LaneMask vac_a = kDense ? 0 : __builtin_amdgcn_ballot_w64(ra <= kEpsF);     // r < 1e-5 (double) for a float32 r
        const LaneMask vac_b = kDense ? 0 : __builtin_amdgcn_ballot_w64(rb <= kEpsF);
        const LaneMask calm_a = __builtin_amdgcn_ballot_w64(own_calm(ua, qa, A.s32, half_um, calm_thr));
        const LaneMask calm_b = __builtin_amdgcn_ballot_w64(own_calm(ub, qb, B.s32, half_um, calm_thr));
        const LaneMask vac_n = vac_a >> 1, calm_n = calm_a >> 1;
        const double uad = (double)ua, ubd = (double)ub, und = (double)un;
        o.easy1 = own_iface<kDense>(rda, yda, ua, uad, A, vac_a, vac_b, ub, ubd, kc, o.Fr1, o.Fy1, o.fp1) & calm_a & calm_b;
        o.triv2 = own_iface<kDense>(rdb, ydb, ub, ubd, B, vac_b, vac_n, un, und, kc, o.Fr2, o.Fy2, o.fp2) & calm_b & calm_n;
    }
}

// grid = L / kG workgroups of kG traffic lanes; block = 64 kG W threads (W = N / 128 wavefronts per lane); dynamic LDS = kG regions.
// kFairShift: steps per turn (2^kFairShift) of the priority rotation between the two halves of the grid (above).
constexpr int kFairShift = 3;
// kSched: `ghost` is a boundary schedule [T][L][2][4] (dhts_macro_rollout_fwd_sched).  Only phase 2 reads the boundary records, so the
// threads m < 2 that wrote them rewrite them in phase 1 of every step n >= 1 -- between the barrier behind phase 2 of step n - 1 and the
// one in front of phase 2 of step n: no further barrier -- from a row that has been in registers since step n - 1, and then load row n + 1:
// the load has a whole step to arrive and never stands between a wavefront and its barrier.  The row waits as ONE register: thread t < 8
// of the lane's LAST wavefront holds element t and the row's address is a scalar (a float4 and a pointer per thread spilled the kernel);
// v_readlane hands the eight values to the two writers.  The last wavefront, because vector memory operations retire in order: the wait
// for the row also waits for all but a few of the wavefront's tape stores issued behind the load, and the last wavefront's youngest ones
// are its phase-1 entries, a whole phase 2 old -- the first wavefront has just stored the step's exceptions.
// kTaps: detector taps (macro_kernels.hip, "detector taps").  The threads are dealt as in phase 2 -- thread g works for lane g % kG of the
// group -- but from the far end: it takes detector slot 64 Wl - 1 - g / kG (+ 64 Wl for a further one, D > N / 2 only) and reads that
// cell's record in phase 2 of step n: the state after step n - 1, which phase 1 has just written and nobody writes again before the
// barrier behind phase 2.  ONE vector register (det_own) and one scalar flag (tap_wave) live across the step loop; everything else is
// formed again from the thread index where it is used (behind an empty asm, so that the compiler does not hoist it out of the step loop
// into registers the kernel does not have: hoisted, the config-2 instantiation spilled 4 registers; like this it has none).
template <int kG, bool kTape, bool kSched = false, bool kTaps = false>
__global__ __launch_bounds__(1024) void macro_rollout_fwd3_kernel(
    int L, int N, int T, double dt, double dx, double um,
    const float *__restrict__ r_in, const float *__restrict__ y_in, const float *__restrict__ u_in,
    const float *__restrict__ q_in, const float *__restrict__ ghost,
    float *__restrict__ r_out, float *__restrict__ y_out, float *__restrict__ u_out, float *__restrict__ q_out,
    float4 *__restrict__ tape, dhts_error *err, int rotate,
    const int32_t *__restrict__ det, int n_det, float *__restrict__ taps) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const int t = tid & 63;
    const int wv = tid >> 6;
    const int Wc = blockDim.x >> 6;                  // wavefronts of the workgroup
    const int Wl = Wc / kG;                          // wavefronts per traffic lane (N = 128 Wl)
    const int sub = wv / Wl;                         // which lane of the group (wave-uniform)
    const int wl = wv - sub * Wl;
    const int lane = kG * blockIdx.x + sub;
    const int H = N >> 1;
    const int m = (wl << 6) + t;                     // this thread's pair: cells 2m, 2m + 1; interfaces 2m + 1, 2m + 2
    const size_t base = (size_t)lane * N;
    const size_t reg = fwd3_region_bytes(N);
    auto region_cr = [&](int s_) { return reinterpret_cast<CellRec *>(smem + (size_t)s_ * reg); };
    auto region_fxe = [&](int s_) { return reinterpret_cast<double2 *>(region_cr(s_) + (N + 2)); };
    auto region_q = [&](int s_) { return reinterpret_cast<int *>(region_fxe(s_) + (N + 1)); };
    auto region_cnt = [&](int s_) { return region_q(s_) + (N + 2); };
    CellRec *CRa = region_cr(sub) + m;               // record of cell 2m
    CellRec *CRb = region_cr(sub) + (H + 2 + m);     // record of cell 2m + 1
    double2 *FXe = region_fxe(sub) + m;              // FXe[0] = interface 2m, FXe[1] = interface 2m + 2
    double2 *FXo = region_fxe(sub) + (H + 1 + m);    // interface 2m + 1
    int *Q = region_q(sub);
    int *CNT = region_cnt(sub);
    IfaceConst kc;
    kc.set_um(um); kc.set_grid(dt, dx);
    const float umf = (float)um;

    // the thread's own cells: float32 state (step 0: as given; later: what the update leaves) and the widened (r, y)
    float ra, ya, ua, qa, rb, yb, ub, qb;
    {
        const float2 r2 = *reinterpret_cast<const float2 *>(r_in + base + 2 * m), y2 = *reinterpret_cast<const float2 *>(y_in + base + 2 * m);
        const float2 u2 = *reinterpret_cast<const float2 *>(u_in + base + 2 * m), q2 = *reinterpret_cast<const float2 *>(q_in + base + 2 * m);
        ra = r2.x; rb = r2.y; ya = y2.x; yb = y2.y; ua = u2.x; ub = u2.y; qa = q2.x; qb = q2.y;
    }
    double rda = (double)ra, yda = (double)ya, rdb = (double)rb, ydb = (double)yb;
    {
        CellPre ca, cb;
        arz_cell_pre(rda, um, ca);
        arz_cell_pre(rdb, um, cb);
        CRa->st = make_float4(ra, ya, ua, qa); CRa->sh = make_double2(ca.s, ca.h); CRa->q0 = make_double2(ca.q0, 0.);
        CRb->st = make_float4(rb, yb, ub, qb); CRb->sh = make_double2(cb.s, cb.h); CRb->q0 = make_double2(cb.q0, 0.);
    }
    if (m < 2) {                                     // the ghosts: m = 0 the left one (slot H + 1), m = 1 the right one (slot H)
        const float *g = ghost + (size_t)lane * 8 + (m ? 4 : 0);
        const float4 st = make_float4(g[0], g[1], g[2], g[3]);
        CellPre c;
        arz_cell_pre((double)st.x, um, c);
        CellRec *gr = region_cr(sub) + (m ? H : H + 1);
        gr->st = st; gr->sh = make_double2(c.s, c.h); gr->q0 = make_double2(c.q0, 0.);
    }
    // the queue's standing entries 0 .. Wl: interfaces 0, 128, ..., N
    const int n_forced = Wl + 1;
    if (m <= Wl) Q[m] = 128 * m;
    if (m == 0) { CNT[0] = n_forced; CNT[1] = n_forced; }
    __syncthreads();

    const TapeGeom geo = tape_geom(N);
    const double c = dt / dx;
    int fault_step = -1, fault_index = 0, fault_lane = 0;
    const float half_um = 0.5f * umf, calm_thr = own_calm_thr(kc);
    const bool young = rotate != 0 && blockIdx.x >= (gridDim.x >> 1);      // (DHTS_OPT_MACRO_FWD_ROTATE: the rotation is for speed only)
    float4 *tp_pair = kTape ? tape + (size_t)(kG * blockIdx.x) * geo.row_f4 : nullptr;     // the group's first row of the step
    const size_t tp_stride = (size_t)L * geo.row_f4;
    const int row_span = (int)(16 * (size_t)kG * geo.row_f4);      // bytes of the group's rows of a step: what the step's buffer descriptor covers
    // the thread's two S slots as byte offsets from the group's first row (interface N has none: that thread's second entry
    // goes onto its first slot and is overwritten)
    const unsigned ts_off1 = (unsigned)(16 * (size_t)sub * geo.row_f4) + 12u * (unsigned)(2 * m + 1);
    const unsigned ts_off2 = (2 * m + 2 < N) ? ts_off1 + 12u : ts_off1;
    // phase 2: this thread's queue (lane s2 of the group), its slot k2 in it (+ blockDim / kG per further round), and where slot
    // k2's exception goes in the lane's row
    const int s2 = tid & (kG - 1), k2 = tid / kG;
    int *q2 = region_q(s2);
    const int *cnt2p = region_cnt(s2);
    typedef __attribute__((address_space(3))) char LdsByte;      // (32-bit pointers: the offsets below stay 32-bit arithmetic)
    const LdsByte *cr2_lds = (const LdsByte *)region_cr(s2);
    LdsByte *fx2_lds = (LdsByte *)region_fxe(s2);
    const unsigned rec_even = (unsigned)sizeof(CellRec) * (unsigned)(H + 1);      // bytes from slot kk to slot H + 1 + kk
    const unsigned offH2 = (unsigned)(16 * ((size_t)s2 * geo.row_f4 + geo.s_f4));

#ifdef DHTS_FWD3_STAMPS
    long long st_last_ = __builtin_amdgcn_s_memtime(), st_acc_[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const long long clk0_ = __builtin_amdgcn_s_memtime(), rt0_ = __builtin_amdgcn_s_memrealtime();
#endif
    float sched_v = 0.f;
    const float *sched_row = nullptr;                // (wave-uniform) the lane's row of the next step
    const bool sched_wave = kSched && __builtin_amdgcn_readfirstlane(wl) == Wl - 1;
    if constexpr (kSched) {
        sched_row = ghost + ((size_t)L + (size_t)__builtin_amdgcn_readfirstlane(lane)) * 8;
        if (sched_wave && t < 8 && T > 1) sched_v = sched_row[t];
    }
    int det_own = -1;
    bool tap_wave = false;
    if constexpr (kTaps) {
        const int j0 = (Wl << 6) - 1 - tid / kG;
        tap_wave = __builtin_amdgcn_readfirstlane((Wl << 6) - 1 - (tid | 63) / kG) < n_det;      // the wavefront's lowest slot
        if (j0 < n_det) det_own = det[j0];
    }
    auto tap = [&](const int s) {                       // the state after step s, out of the lanes' records
        if (tap_wave) {
            int tl = threadIdx.x;
            asm volatile("" : "+v"(tl));
            const int sl = tl & (kG - 1);
            const CellRec *cr = region_cr(sl);
            const int Hh = H;
            float *row = taps + ((size_t)s * L + (size_t)(kG * blockIdx.x + sl)) * 3 * n_det;
            taps_write(det, n_det, det_own, (Wl << 6) - 1 - tl / kG, Wl << 6, N, row,
                       [=](unsigned dc) { return cr[(dc & 1u) ? Hh + 1 + ((dc + 1u) >> 1) : (dc >> 1)].st; });
        }
    };
    auto body = [&](auto upd_c, auto solve_c, const int n) {
        constexpr bool upd = decltype(upd_c)::value;       // finish step n - 1
        constexpr bool solve = decltype(solve_c)::value;   // start step n
        if constexpr (kSched && upd && solve) {
            if (sched_wave) {
                float e[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) e[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sched_v), k));
                if (t < 2) {
                    const float4 st = t ? make_float4(e[4], e[5], e[6], e[7]) : make_float4(e[0], e[1], e[2], e[3]);
                    CellPre cg;
                    arz_cell_pre((double)st.x, um, cg);
                    CellRec *gr = region_cr(sub) + (t ? H : H + 1);
                    gr->st = st; gr->sh = make_double2(cg.s, cg.h); gr->q0 = make_double2(cg.q0, 0.);
                }
                sched_row += (size_t)L * 8;
                if (t < 8 && n + 1 < T) sched_v = sched_row[t];
            }
        }
        char *row0 = reinterpret_cast<char *>((kTape && solve) ? tp_pair : nullptr);
        if (kTape) tp_pair += tp_stride;
        int *cnt = CNT + (n & 1);
        if (solve) {
            if (young && ((n >> kFairShift) & 1)) __builtin_amdgcn_s_setprio(1);
            else __builtin_amdgcn_s_setprio(0);
        }
        // ---- phase 1 ----
        OwnPre A, B;
        PairOut po;
        if (upd) {
            // Godunov update, _macro_lane.py:109-112, float32 store :327-334
            const double2 F0 = FXe[0], F1 = FXo[0], F2 = FXe[1];
            ra = (float)(rda + (F0.x - F1.x) * c);
            ya = (float)(yda + (F0.y - F1.y) * c);
            rb = (float)(rdb + (F1.x - F2.x) * c);
            yb = (float)(ydb + (F1.y - F2.y) * c);
            rda = (double)ra; yda = (double)ya; rdb = (double)rb; ydb = (double)yb;
        } else {
            own_pre_init(rda, kc, A);
            own_pre_init(rdb, kc, B);
        }
        // (the dense form needs r > float32(eps) of every cell the wavefront looks at: its own 128 -- the right neighbour of lane
        // 63's second cell only enters an interface that is queued anyway; a NaN takes the general form)
        if (__builtin_amdgcn_ballot_w64((ra <= kEpsF) | (rb <= kEpsF) | !(ra == ra) | !(rb == rb)) == 0) {
            pair_phase1<true, upd, solve>(ra, ya, rb, yb, rda, yda, rdb, ydb, ua, qa, ub, qb, A, B, CRa, CRb, umf, half_um, calm_thr, kc, po);
        } else {
            asm volatile("" ::: "memory");
            pair_phase1<false, upd, solve>(ra, ya, rb, yb, rda, yda, rdb, ydb, ua, qa, ub, qb, A, B, CRa, CRb, umf, half_um, calm_thr, kc, po);
        }
        if (!solve) {
            *reinterpret_cast<float2 *>(r_out + base + 2 * m) = make_float2(ra, rb);
            *reinterpret_cast<float2 *>(y_out + base + 2 * m) = make_float2(ya, yb);
            *reinterpret_cast<float2 *>(u_out + base + 2 * m) = make_float2(ua, ub);
            *reinterpret_cast<float2 *>(q_out + base + 2 * m) = make_float2(qa, qb);
            if constexpr (kTaps && upd) {               // the final step writes no records: the state once more, for the taps
                CRa->st = make_float4(ra, ya, ua, qa);
                CRb->st = make_float4(rb, yb, ub, qb);
                lds_only_barrier();
                tap(n - 1);
            }
            return;
        }
        // (lane masks from here to the barrier: who stores a flux, who appends one entry or two -- scalar logic, the vector side sees
        // EXEC masks and one select for the atomic's operand.  Lane 63's second interface is a standing entry: never appended.)
        const LaneMask last_m = 1ull << 63;
        const LaneMask app1_m = ~po.easy1, app2_m = ~(po.triv2 | last_m);
        const bool app1 = __builtin_amdgcn_inverse_ballot_w64(app1_m), app2 = __builtin_amdgcn_inverse_ballot_w64(app2_m);
        if (__builtin_amdgcn_inverse_ballot_w64(po.easy1)) FXo[0] = make_double2(po.Fr1, po.Fy1);
        if (__builtin_amdgcn_inverse_ballot_w64(po.triv2 & ~last_m)) FXe[1] = make_double2(po.Fr2, po.Fy2);
        // the queue: one LDS atomic per thread that has something to append
        const int nq = __builtin_amdgcn_inverse_ballot_w64(app1_m & app2_m) ? 2 : 1;      // (where the thread appends at all)
        int kq = 0;
        if (__builtin_amdgcn_inverse_ballot_w64(app1_m | app2_m)) kq = atomicAdd(cnt, nq);
        // The tape row as a buffer: the group's first row of the step is the descriptor's base (scalar), a thread's place in it a 32-bit
        // offset -- no 64-bit vector add per store; a store past the group's rows would be dropped, not written.
        const __amdgpu_buffer_rsrc_t trow = __builtin_amdgcn_make_buffer_rsrc(row0, 0, kTape ? row_span : 0, 0x00020000);
        if (kTape) {
            __builtin_amdgcn_raw_buffer_store_b96(fp_tape_bits(po.fp2), trow, ts_off2, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b96(fp_tape_bits(po.fp1), trow, ts_off1, 0, 0);
        }
        if (app1) Q[kq] = 2 * m + 1;
        if (app2) Q[kq + nq - 1] = 2 * m + 2;                  // the thread's last slot: behind its first entry if it appended one
        FWD3_STAMP(0)
        lds_only_barrier();
        FWD3_STAMP(1)
        // ---- phase 2 ----
        int qn2 = cnt2p[n & 1];
        bool held = false;
        for (int k = k2; ; k += blockDim.x / kG) {
            unsigned i = (unsigned)q2[k < N + 2 ? k : 0];             // read beside the count, not behind it:
            asm volatile("" : "+v"(i), "+v"(qn2));                    // (both loads issued, ONE wait; unpinned, the entry's load sinks behind the branch on the count)
            if (!(k < qn2)) break;
            if (!held) { held = true; __builtin_amdgcn_s_setprio(3); }      // the workgroup's critical path
            // The records of interface i = 2 kk + odd: left cell in slot kk (odd) or H + 1 + kk (even), right cell in slot H + 2 + kk (odd)
            // or kk (even); its flux in slot kk + odd (H + 1).  Formed as 32-bit LDS byte offsets with 24-bit multiply-adds: indexing the
            // generic pointers costs three 64-bit multiply-adds and a select chain in front of the reads.  __umul24 needs both factors
            // below 2^24: they are kk <= H, odd <= 1, 48 and 48 (H + 2) -- and H <= 1024, because a lane has N / 128 <= 16 wavefronts under
            // __launch_bounds__(1024) and its region must fit the 160 KB of LDS (dhts_macro_rollout_plan refuses the kernel otherwise).
            const unsigned kk = i >> 1, odd = i & 1u;
            const unsigned rec_kk = __umul24(kk, (unsigned)sizeof(CellRec));
            const unsigned left_off = rec_kk + rec_even - __umul24(odd, rec_even), right_off = rec_kk + __umul24(odd, rec_even + (unsigned)sizeof(CellRec));
            const CellRec *lf = (const CellRec *)(cr2_lds + left_off), *rt = (const CellRec *)(cr2_lds + right_off);
            const float4 ls = lf->st, rs = rt->st;
            const double2 lsh = lf->sh;
            Iface f;
            const LaneMask bad_m = arz_interface_queued(ls, lsh.x, lsh.y, lf->q0.x, rs, rt->sh.y, kc, f);
            *(double2 *)(fx2_lds + (16u * kk + __umul24(odd, 16u * (unsigned)(H + 1)))) = make_double2(f.Fr, f.Fy);
            if (kTape) {
                typedef unsigned v2u __attribute__((ext_vector_type(2)));
                if (k == 0) __builtin_amdgcn_raw_buffer_store_b64(v2u{(unsigned)qn2, 0u}, trow, offH2, 0, 0);
                __builtin_amdgcn_raw_buffer_store_b16((unsigned short)i, trow, offH2 + 8u + 2u * (unsigned)k, 0, 0);
                const unsigned offE = offH2 + 16u * (unsigned)geo.h_f4 + 32u * (unsigned)k;
                __builtin_amdgcn_raw_buffer_store_b128(bits_f4(f.A[0], f.A[1], f.A[2], f.A[3]), trow, offE, 0, 0);
                __builtin_amdgcn_raw_buffer_store_b128(bits_f4(f.B[0], f.B[1], f.B[2], f.B[3]), trow, offE + 16u, 0, 0);
            }
            if (bad_m) {
                asm volatile("" ::: "memory");
                if (__builtin_amdgcn_inverse_ballot_w64(bad_m) && fault_step < 0) { fault_step = n; fault_index = (int)i; fault_lane = kG * blockIdx.x + s2; }
            }
        }
        __builtin_amdgcn_s_setprio(0);
        if constexpr (kTaps && upd) tap(n - 1);
        if (tid < kG) region_cnt(tid)[(n + 1) & 1] = n_forced;
#ifdef DHTS_FWD3_STAMPS
        const bool held_ = __builtin_amdgcn_ballot_w64(held) != 0;
        if (held_) { st_acc_[4] += 1; st_acc_[5] += __builtin_popcountll(__builtin_amdgcn_ballot_w64(held)); }
        if (held_) { FWD3_STAMP(2) } else { FWD3_STAMP(6) }
#endif
        lds_only_barrier();
#ifdef DHTS_FWD3_STAMPS
        if (held_) { FWD3_STAMP(3) } else { FWD3_STAMP(7) }
#endif
    };
    using yes = std::integral_constant<bool, true>;
    using no = std::integral_constant<bool, false>;
    if (T == 0) {
        body(no{}, no{}, 0);
    } else {
        body(no{}, yes{}, 0);
        for (int n = 1; n < T; ++n) body(yes{}, yes{}, n);
        body(yes{}, no{}, T);
    }
    if (fault_step >= 0) raise_fault(err, DHTS_FAULT_CFL, fault_step, fault_lane, fault_index);
#ifdef DHTS_FWD3_STAMPS
    // slots 0 .. 7: workgroups 0 .. 7; slots 8 .. 15: workgroups gridDim / 2 .. gridDim / 2 + 7 (dispatched behind the first half)
    const int half_ = (int)(gridDim.x >> 1);
    const int slot_ = (int)blockIdx.x < 8 ? (int)blockIdx.x : (((int)blockIdx.x >= half_ && (int)blockIdx.x < half_ + 8) ? 8 + (int)blockIdx.x - half_ : -1);
    if (slot_ >= 0 && t == 0 && wv < 16)
        for (int j = 0; j < 8; ++j) dhts_fwd3_stamps[slot_][wv][j] = st_acc_[j];
    if (slot_ >= 0 && tid == 0) {
        dhts_fwd_clock[1][slot_][0] = __builtin_amdgcn_s_memtime() - clk0_;
        dhts_fwd_clock[1][slot_][1] = __builtin_amdgcn_s_memrealtime() - rt0_;
    }
#endif
}
