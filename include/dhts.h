/*
 * dhts.h -- C ABI of libdhts.so: the MI355X (gfx950) differentiable traffic stepper.
 *
 * The reference (SonSang/diff-hybrid-traffic-sim) has NO FFI: its hot path sits behind two Python
 * torch.autograd.Function operators,
 *     dMacroForwardLayer   road/lane/dmacro_lane.py:234-309   (ARZ cell stencil, forward + Jacobian tape)
 *     dMicroForwardLayer   road/lane/dmicro_lane.py:228-298   (IDM car-following ODE, forward + tape)
 * each called once per lane per step from RoadNetwork.forward (road/network/road_network.py:99-101).
 * This header is the boundary a maintainer binds instead (ctypes stub in INTEGRATION.md): plain
 * pointers and sizes, no torch types.  Every entry point cites the reference code it replaces.
 *
 * Conventions
 *   - All array pointers are DEVICE pointers owned by the caller (hipMalloc / torch CUDA tensors),
 *     float32 unless stated.  Nothing is allocated, freed or synchronised inside a call; work is
 *     enqueued on `stream` (a hipStream_t passed as void*; NULL = default stream).
 *   - Return value: DHTS_OK, or a negative DHTS_E_* for a host-side failure (bad argument, launch
 *     error).  Simulation faults the reference reports with `assert` (CFL violation
 *     _macro_lane.py:141-146, vehicle collision _micro_lane.py:151-162) are written to the optional
 *     device-side sticky record `dhts_error*` (first fault wins) and read back by the caller after the
 *     rollout; the rollout itself continues the way the reference's arithmetic would.
 *   - Layouts: state planes are [lane][cell] (cell fastest).  The Jacobian tapes are internal to this
 *     library but documented so they can be inspected.  There are two formats per model:
 *       single-step operators (dhts_macro_step_*, dhts_micro_step_*) keep the reference's blocks,
 *         macro: [lane][3][Np][4] float32, Np = dhts_padded(N) (multiple of 64); plane k = 0/1/2 holds
 *                d(next cell a)/d(cell a-1 / a / a+1) as row-major 2x2 in (r, y) -- the reference's
 *                dqs[a][k] (dmacro_lane.py:50-56) with the cell index moved inside for coalescing;
 *         micro: [lane][2][Vp][4] float32; plane 0 = dEgo, plane 1 = dLeading (dmicro_lane.py:48-54);
 *       rollouts (dhts_macro_rollout_*, dhts_micro_rollout_*) keep COMPACT tapes the reverse sweep
 *         rebuilds those blocks from: see dhts_macro_tape_bytes and dhts_micro_tape_bytes below;
 *         dhts_macro_tape_expand writes a rollout's blocks out in the single-step layout.
 */
#ifndef DHTS_H
#define DHTS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DHTS_VERSION 100 /* 0.1.0 */

#define DHTS_OK 0
#define DHTS_E_INVALID (-1)   /* bad argument (NULL where required, non-positive size, unsupported size) */
#define DHTS_E_LAUNCH (-2)    /* HIP launch / runtime error */
#define DHTS_E_NO_DEVICE (-3) /* no gfx950 device visible */

/* fault codes in dhts_error.code */
#define DHTS_FAULT_NONE 0
#define DHTS_FAULT_CFL 1       /* dt >= dx / max(|speed|, 1e-5) at an interface  (_macro_lane.py:141-146) */
#define DHTS_FAULT_COLLISION 2 /* gap to the leader < 0                           (_micro_lane.py:151-162) */
#define DHTS_FAULT_NAN 3       /* non-finite cotangent in the reverse sweep       (dmacro_lane.py:308)     */
#define DHTS_FAULT_CAPACITY 4  /* hybrid network: record stream / vehicle slots / lane list / route table exhausted */

typedef struct dhts_error {
    int32_t code;  /* DHTS_FAULT_*; 0 = no fault.  Caller zeroes it before the first call. */
    int32_t step;  /* step index within the rollout */
    int32_t lane;  /* lane index */
    int32_t index; /* interface / vehicle index within the lane */
} dhts_error;

/* ---- macro (ARZ) ------------------------------------------------------------------------------- */
typedef struct dhts_macro_desc {
    int32_t n_lanes;  /* L: independent lanes in the batch */
    int32_t n_cells;  /* N: cells per lane (1 .. DHTS_MACRO_MAX_CELLS) */
    double dt;        /* delta_time */
    double dx;        /* cell_length (MacroLane.cell_length, _macro_lane.py:44) */
    double u_max;     /* speed_limit */
} dhts_macro_desc;

#define DHTS_MACRO_MAX_CELLS 4000

int dhts_version(void);
/* number of visible gfx950 devices, or DHTS_E_NO_DEVICE */
int dhts_device_count(void);
/* tuning knobs (process-wide, not part of the numerical contract).
 * DHTS_OPT_MACRO_FWD_WAVES: wavefronts per traffic lane in the macro forward kernel, 1..16 (the single-step operator's
 * kernel uses at most 8); 0 = heuristic. */
#define DHTS_OPT_MACRO_FWD_WAVES 1
/* DHTS_OPT_MICRO_FWD_WAVES: wavefronts per traffic lane in the micro forward kernel, 1, 2 or 4; 0 = heuristic. */
#define DHTS_OPT_MICRO_FWD_WAVES 2
/* DHTS_OPT_MACRO_FWD_VARIANT: kernel behind dhts_macro_rollout_fwd: 0 = two-phase kernels (trivial interfaces solved in
 * place, the others queued and solved compacted; full lanes of 128 W cells without a history take the pair kernel -- a thread owns
 * two adjacent cells and their right interfaces), 1 = the one-phase kernel of dhts_macro_step_fwd (every interface an
 * exception), 2 = the two-phase LANE kernel for every shape (one cell and its left interface per thread-pass, one lane per
 * workgroup: what ragged lanes and state histories take anyway; selectable so that tests can hold the pair kernel to it).
 * Same tape format, same results. */
#define DHTS_OPT_MACRO_FWD_VARIANT 3
/* DHTS_OPT_MACRO_FWD_GROUP: traffic lanes per workgroup of the pair kernel: 0 = heuristic (default: 4 for lanes of up to three
 * wavefronts, 1 for lanes of four -- BASELINE config 2 --, 2 above), or 1, 2, 4 (taken where the lanes divide, the launch keeps
 * >= 256 workgroups and the group fits a workgroup and the LDS).  Same results, same tape (dhts_macro_rollout_plan plan[7] says
 * what a shape gets). */
#define DHTS_OPT_MACRO_FWD_GROUP 4
/* DHTS_OPT_MACRO_FWD_ROTATE: 1 (default) = the workgroups of the second half of the pair kernel's grid take turns with the others at
 * issue priority 1, eight steps at a time; 0 = nobody does.  The rotation rests on an OBSERVATION about the dispatcher (workgroups b
 * and b + grid / 2 share a compute unit at two workgroups per unit, and the one dispatched second loses the arbitration), is used for
 * speed only and changes no result; bench.py times both settings during its warm-up and reports which one the box prefers. */
#define DHTS_OPT_MACRO_FWD_ROTATE 5
/* DHTS_OPT_NETSTEP_LDS_KB: KB of LDS the persistent kernels of dhts_netstep_rollout_* may plan with for what they keep resident (static
 * tables + per-step rows + ghosts, the micro side's running state, state rows / cotangent planes: dropped in that order of priority when
 * they do not fit); 1 .. 158, 0 = default (158).  Chooses among instantiations that compute the same numbers -- the tests run them all. */
#define DHTS_OPT_NETSTEP_LDS_KB 6
/* DHTS_OPT_NETSTEP_BLOCK: threads per workgroup of the persistent kernels: 256, 512, 1024; 0 = heuristic.  Same results. */
#define DHTS_OPT_NETSTEP_BLOCK 7
/* DHTS_OPT_HYB_PACK: replicas per compute unit of the fused hybrid network kernels (dhts_net_hybrid_rollout_fwd / _bwd): 0 = one;
 * 1 = two whenever the plan fits (half the LDS per workgroup: a smaller record staging area, temporaries for the network's own
 * micro lanes only; the 128-register instantiation); 2 (default) = two when the batch has more replicas than the device has
 * compute units.  Same results bit for bit; the value must not change between a forward sweep and its reverse (the reverse
 * sweep raises DHTS_FAULT_CAPACITY with index -3 otherwise).  dhts_net_hybrid_plan tells what a launch would take. */
#define DHTS_OPT_HYB_PACK 8
/* DHTS_OPT_REWARD_CHAIN: 1 = every network rollout (dhts_net_macro_rollout_fwd / _eval, dhts_net_hybrid_rollout_fwd / _eval,
 * dhts_netstep_rollout_fwd) finishes with the reward as ItscpEnv._reward forms it (example/control/itscp/_env.py:770-797): ONE
 * running float32 sum over lanes (outermost) and steps -- L x T dependent additions, one wavefront per replica, ~0.4 ms at config 4
 * -- instead of the kernels' own order (a lane's steps first, then the lanes' subtotals: the same real number, another
 * float32 rounding, 6e-6 relative at config 4).  An evaluation episode follows the reference's mixed chain (a Python float
 * until the first cell lane's tensor term joins it).  0 (default).  The queue terms and the gradient are the same either way. */
#define DHTS_OPT_REWARD_CHAIN 9
/* DHTS_OPT_MACRO_JVP_VARIANT: kernel behind dhts_macro_rollout_jvp: 0 = heuristic (one cell per thread with the tangents in registers
 * for lanes of 2 .. 1024 cells, the general kernel otherwise), 1 = the general kernel for every shape (tests hold the fast kernel to it).
 * Same results bit for bit.  (Option 10 is not assigned: dhts_set_option(10, ...) is DHTS_E_INVALID, as for every unknown option.) */
#define DHTS_OPT_MACRO_JVP_VARIANT 11
int dhts_set_option(int option, int value);
/* cells / vehicle slots rounded up to the tape's padded width (multiple of 64) */
int dhts_padded(int n);
/* bytes of Jacobian tape for T fused steps (dhts_macro_rollout_*).  The rollout tape holds, per (step, lane) row, what the
 *   reverse sweep needs to form the interface products A_i = flux'(Q_0) dQ_0/dQ_L, B_i = flux'(Q_0) dQ_0/dQ_R (the two 2x2
 *   products of dMacroLane._backward, dmacro_lane.py:116-124) of every interface i = 0 .. n_cells.  ROW LAYOUT (three
 *   blocks, each rounded up to a whole number of 128-byte lines; tests/test_boundary.py parses the three lines below):
 *     S: float32 [n_cells][3]                     (fp[0], fp[2], fp[3]) of interface i < n_cells, valid where it is trivial
 *     H: uint32 cnt, uint32 0, uint16 idx[n_cells + 1]   idx[j] = the interface of exception j < cnt
 *     E: float32 [n_cells + 1][2][4]              (A, B) of exception j; only the first cnt entries are written and read
 *   Where Q_0 = Q_L (the trivial Riemann case) dQ_0/dQ_L = I and dQ_0/dQ_R = 0, so A_i is the flux Jacobian fp at Q_L
 *   (darz.py:217-233), whose entry [0][1] is the constant 1, and B_i = 0: three floats.  Every other interface -- Q_0 is not
 *   Q_L, or the forward kernel chose to solve it in full; interface n_cells always -- is an "exception" and keeps its two
 *   products in E, in the order the forward solved them (its S entry is then unspecified).  There is no bit mask: a reader
 *   marks the interfaces listed in idx[0 .. cnt) and treats the rest as trivial.  The reverse sweep forms the reference's
 *   cell blocks dqs[a][0] = c A_a, dqs[a][1] = I - c (A_{a+1} - B_a), dqs[a][2] = - c B_{a+1} (c = dt / dx;
 *   dmacro_lane.py:126-129) from the products with the same float32 operations, so the results are those of the 48-byte
 *   per-cell tape; dhts_macro_tape_expand writes them out.
 *   The row is sized for the worst case (every interface an exception); the bytes MOVED per row are 12 n_cells + 8 +
 *   2 cnt + 32 cnt rounded to lines (BASELINE config 2: cnt ~ 0.15 n_cells, 8.8 KB per 512-cell row against 24.6 KB of
 *   dqs blocks). */
size_t dhts_macro_tape_bytes(const dhts_macro_desc *d, int T);
/* the reference's blocks dqs[a][3][2][2] (dmacro_lane.py:56) of all T steps from a rollout tape, in the single-step operator's
 *   layout per step: dqs_out [T][lane][3][Np][4] float32 (T x dhts_macro_step_tape_bytes).  For tests and for callers that want
 *   the Jacobians themselves; the reverse sweep does not need it. */
int dhts_macro_tape_expand(const dhts_macro_desc *d, int T, const float *tape, float *dqs_out, void *stream);
/* bytes of the single-step operator's tape (dhts_macro_step_*): the reference's per-cell blocks
 *   [lane][3][Np][4] float32, Np = dhts_padded(n_cells): plane k holds dqs[a][k] of every cell a */
size_t dhts_macro_step_tape_bytes(const dhts_macro_desc *d);

/*
 * n independent cell interfaces: ARZ.riemann_solve (model/macro/_arz.py:212-332) + dARZ.compute_dLdR and
 * dARZ.flux_prime (model/macro/darz.py:194-233) + the two 2x2 products of dMacroLane._backward
 * (road/lane/dmacro_lane.py:126-129), exactly as the rollout kernel evaluates them per interface.
 *   in  [9][n] DOUBLE (SoA): rL yL uL ueqL rR yR uR ueqR u_max  (float32-valued state widened to double)
 *   variant 0 = production arithmetic, 1 = reference-order IEEE division / square root
 *   out case_ind [n] int32 (0 = Q_L, 1 = Q_M, 2 = Q_C); q0 [4][n] DOUBLE (r, y, u, u_eq of Q_0);
 *       flux [2][n] DOUBLE (r u, y u of Q_0); dL, dR, fp [4][n] float32 row-major 2x2; A = fp @ dL, B = fp @ dR [4][n];
 *       cfl_bad [n] int32 = the CFL assert of _macro_lane.py:141-146 would fire for (dt, dx);
 *       speed [2][n] DOUBLE or NULL = (speed0, speed1) as ARZ.riemann_solve returns them (_arz.py:316-332), reference-order
 *       arithmetic in both variants (the rollout kernels only test them against the CFL bound)
 */
int dhts_arz_interface_batch(int64_t n, int variant, const double *in, double dt, double dx, int32_t *case_ind, double *q0,
                             double *flux, float *dL, float *dR, float *fp, float *A, float *B, int32_t *cfl_bad, double *speed,
                             void *stream);

/* float32 glue of FullQ.set_r_u / FullQ.from_r_u (model/macro/_arz.py:73-86 with :121-138):
 * y = r * (u - u_eq(r)), u_eq = u_max * (1 - sqrt(max(r, 0) + 1e-5)); n elements. */
int dhts_macro_state_from_ru(int64_t n, double u_max, const float *r, const float *u, float *y, float *ueq, void *stream);
/* its adjoint as torch autograd evaluates it: g_r += g_y * d y/d r, g_u = g_y * r   (g_r in/out, g_u out) */
int dhts_macro_state_from_ru_bwd(int64_t n, double u_max, const float *r, const float *u, const float *g_y,
                                 float *g_r, float *g_u, void *stream);
/* adjoint of the speed tap u = y / max(r, eps) + u_eq(max(r, eps)) of FullQ.set_r_y (_arz.py:88-92,126-131):
 * g_r += g_u * d u/d r, g_y += g_u * d u/d y   (both in/out) */
int dhts_macro_u_tap_bwd(int64_t n, double u_max, const float *r, const float *y, const float *g_u,
                         float *g_r, float *g_y, void *stream);

/*
 * T fused steps of L independent lanes: replaces T x L calls of dMacroForwardLayer.forward
 * (dmacro_lane.py:236-275 = MacroLane.forward _macro_lane.py:83-146 + dMacroLane._backward :96-132 +
 * the float32 u/u_eq glue of set_next_state_vector_y _macro_lane.py:282-299).
 *   in : r, y, u, ueq [L][N]; ghost [L][2][4] = per lane (left, right) x (r, y, u, ueq), constant over the
 *        rollout (RoadNetwork.setup_macro_boundary for a lane without neighbours, road_network.py:299-387)
 *   out: r_out, y_out, u_out, ueq_out [L][N] (may alias the inputs);
 *        tape (dhts_macro_tape_bytes) or NULL for a non-differentiable run;
 *        hist [T][L][3][N] = (r, y, u) after every step, or NULL
 */
int dhts_macro_rollout_fwd(const dhts_macro_desc *d, int T,
                           const float *r, const float *y, const float *u, const float *ueq, const float *ghost,
                           float *r_out, float *y_out, float *u_out, float *ueq_out,
                           float *tape, float *hist, dhts_error *err, void *stream);
/*
 * Reverse sweep over the tape: replaces T x L calls of dMacroForwardLayer.backward (dmacro_lane.py:277-309).
 *   in : g_r, g_y [L][N] cotangent of the final (r, y); g_hist [T][L][2][N] optional cotangent of the
 *        (r, y) after every step (NULL = none)
 *   out: g_r_out, g_y_out [L][N] cotangent of the initial (r, y) (may alias the inputs);
 *        g_ghost [L][2][2] DOUBLE = per lane (left, right) x (r, y): sum over steps of the cotangent that
 *        reaches the ghost cells (grad_ry[0], grad_ry[-1] of dmacro_lane.py:302-303)
 */
int dhts_macro_rollout_bwd(const dhts_macro_desc *d, int T, const float *tape,
                           const float *g_r, const float *g_y, const float *g_hist,
                           float *g_r_out, float *g_y_out, double *g_ghost, dhts_error *err, void *stream);

/*
 * The same rollout with TIME-VARYING boundary cells (set_leftmost_cell / set_rightmost_cell with fresh tensors in front of every
 * RoadNetwork.forward) and the cotangent of every step's boundary cells.  Everything else -- state planes, tape format and
 * dhts_macro_tape_bytes, hist / g_hist, the fault record (a CFL fault carries step, lane and interface), the plan below -- is that of the
 * two calls above, and with ghost_sched[t] = ghost for every t the states, hist, the tape and g_r_out / g_y_out are theirs bit for bit.
 *   ghost_sched   [T][L][2][4] float32 = per step and lane (left, right) x (r, y, u, ueq): step t (the step that turns the state after t
 *                 steps into the state after t + 1) reads row t and no other.  float32 cells only: the double "source" encoding of
 *                 dhts_macro_step_fwd is not decoded here (a NaN density is taken as a NaN density).
 *   g_ghost_sched [T][L][2][2] DOUBLE = per step and lane (left, right) x (r, y): row t is the cotangent that reaches the boundary cells
 *                 of step t, i.e. exactly the addend dhts_macro_rollout_bwd adds into g_ghost at that step (a float32 value, widened);
 *                 the rows added up newest step first give g_ghost bit for bit.  Every row is written (plain stores, no atomics: two
 *                 runs give the same bits); g_hist as above.
 * T = 0 is accepted (no row is read or written).  NULL ghost_sched / g_ghost_sched or a bad descriptor: DHTS_E_INVALID, nothing is
 * dereferenced.
 */
int dhts_macro_rollout_fwd_sched(const dhts_macro_desc *d, int T,
                                 const float *r, const float *y, const float *u, const float *ueq, const float *ghost_sched,
                                 float *r_out, float *y_out, float *u_out, float *ueq_out,
                                 float *tape, float *hist, dhts_error *err, void *stream);
int dhts_macro_rollout_bwd_sched(const dhts_macro_desc *d, int T, const float *tape,
                                 const float *g_r, const float *g_y, const float *g_hist,
                                 float *g_r_out, float *g_y_out, double *g_ghost_sched, dhts_error *err, void *stream);

/* Which kernel instantiations the calls above launch for this shape and the current options -- the _sched forms take the same ones,
 * compiled for a schedule -- (answered by the functions the launches themselves call; tests pin the benchmarked instantiations with it):
 *   plan[0] forward kernel: 0 = two-phase lane kernel, 1 = one-phase, 2 = two-phase pair kernel
 *   plan[1] wavefronts per lane     plan[2] 64-cell passes per wavefront (pair kernel: two adjacent cells per thread)
 *   plan[3] 1 = the full-lane, history-free instantiation (n_cells = 64 x passes x wavefronts and hist == NULL)
 *   plan[4] reverse kernel: 1 = pipelined one-cell-per-thread, 2 = pipelined two-cells-per-thread, 0 = general     plan[5] its block size
 *   plan[6] 1 = per-step cotangents / history requested (want_hist)
 *   plan[7] traffic lanes per workgroup (the pair kernel: DHTS_OPT_MACRO_FWD_GROUP; 1 otherwise) */
int dhts_macro_rollout_plan(const dhts_macro_desc *d, int T, int want_hist, int32_t plan[8]);

/*
 * The same rollout with DETECTOR TAPS: the state at a few chosen cells after every step, and its cotangent, without a history.
 * Replaces get_state_vector read at chosen cells after every RoadNetwork.forward, as the inverse examples do with loop-detector
 * readings (example/inverse/macro.py:34-68, _inverse.py:91-99), where hist / g_hist would move [T][L][N] planes for a handful of cells.
 *   det    [n_det] int32, DEVICE memory, shared by all lanes: cell indices, strictly ascending, in [0, n_cells); 1 <= n_det <= n_cells.
 *   taps   [T][L][3][n_det] float32 = (r, y, u) of cell det[j] after every step: exactly what hist[t][l][:][det[j]] would hold.  Plain
 *          stores, no atomics; every element is written when T > 0 and the indices are valid; two runs give the same bits.
 *   g_taps [T][L][2][n_det] float32 = cotangent of those (r, y); added to the cell's cotangent where and when g_hist is added, so that
 *          g_r_out / g_y_out / g_ghost equal those of a g_hist that is zero outside the detector columns.
 *   ghost / g_ghost: [L][2][4] / [L][2][2] DOUBLE (g_ghost may be NULL) when ghost_is_sched == 0 -- the semantics of
 *          dhts_macro_rollout_fwd / _bwd --, the schedules [T][L][2][4] / [T][L][2][2] of the _sched pair when it is 1 (g_ghost required).
 * There is no hist in this form (a caller who wants every cell has it in the calls above).  Tape format, dhts_macro_tape_bytes and the
 * fault record are those of the calls above; T = 0 is accepted (no row is read or written, the state comes back as it went in).
 * INDEX CONTRACT: the entry points cannot look at the contents of det without a synchronisation and do not; the kernels are safe by
 * construction instead.  Every entry is compared against [0, n_cells) before any address, global or LDS, is formed from it; an entry
 * outside matches no cell: its column of taps is not written and its column of g_taps is not read.  Entries that repeat or are out
 * of order touch no memory outside the buffers either, but which of two equal entries a reverse sweep reads is then unspecified.
 * NULL det / taps / g_taps, n_det outside 1 .. n_cells or a bad descriptor: DHTS_E_INVALID, nothing is dereferenced.
 * dhts_macro_taps_plan has the fields of dhts_macro_rollout_plan (plan[6] = 0) and IS the plan of the same shape without a history --
 * full lanes of 128 W cells stay on the pair kernel with the same lanes per workgroup, N = block keeps the full reverse instantiation --
 * with one exception: lanes of 1026 .. 2048 cells take the general reverse sweep (plan[4] = 0), as they do with a history; the
 * two-cells-per-thread kernel carries no per-step cotangents.
 */
int dhts_macro_rollout_fwd_taps(const dhts_macro_desc *d, int T,
                                const float *r, const float *y, const float *u, const float *ueq, const float *ghost, int ghost_is_sched,
                                float *r_out, float *y_out, float *u_out, float *ueq_out, float *tape,
                                const int32_t *det, int n_det, float *taps, dhts_error *err, void *stream);
int dhts_macro_rollout_bwd_taps(const dhts_macro_desc *d, int T, const float *tape, const float *g_r, const float *g_y,
                                const int32_t *det, int n_det, const float *g_taps,
                                float *g_r_out, float *g_y_out, double *g_ghost, int ghost_is_sched, dhts_error *err, void *stream);
int dhts_macro_taps_plan(const dhts_macro_desc *d, int T, int n_det, int32_t plan[8]);

/*
 * Forward-mode tangent sweep (Jacobian-vector products) over a rollout tape: n_dir = K directions in one call, oldest step first.
 * The sweep applies the cell blocks the reverse sweep applies transposed (dqs[a][0 .. 2], rebuilt from the tape with the same float32
 * operations; dhts_macro_tape_expand writes them out), row-major 2 x 2 in (r, y):
 *     t'_k = (dqs[k][1] t_k + dqs[k][0] t_{k-1}) + dqs[k][2] t_{k+1},   every 2-term product a float32 multiply + fused multiply-add,
 * with t_{-1} / t_{n_cells} the tangent of the left / right boundary cell of that step.  The tape of a step is read once for up to four
 * directions (launches of 4, then 2, then 1 directions, a remainder of 3 as one launch of 4 with a slot masked: dhts_macro_jvp_plan).  The result of a direction does not depend on K, on its
 * place among the directions or on the kernel that ran it, bit for bit.
 *   t_r, t_y            [K][lane][cell] float32: tangent of the initial (r, y); t_r_out, t_y_out: of the final one (may alias t_r, t_y)
 *   t_ghost             tangent of the boundary cells, (left, right) x (r, y) float32: NULL = zero; [K][lane][2][2] = the same in front
 *                       of every step (ghost_is_sched = 0); [K][T][lane][2][2] = row t read by step t and no other (ghost_is_sched != 0).
 *                       ghost_is_sched != 0 with a NULL t_ghost is DHTS_E_INVALID (zero tangents are NULL with ghost_is_sched = 0).
 *   det, n_det, t_taps  det NULL (then t_taps NULL too): no readings.  Else t_taps [K][T][lane][2][n_det] receives the tangent of (r, y)
 *                       of the cells det[j] AFTER every step, where dhts_macro_rollout_fwd_taps writes taps.  The index contract is the
 *                       taps form's: an entry outside [0, n_cells) is compared away before any address is formed; its column is not written.
 *   err                 the first step after which a thread finds a non-finite tangent raises DHTS_FAULT_NAN (step, lane, cell).
 * T = 0 is accepted: the tangents come back as they went in, no row of anything is read or written.  A bad descriptor, n_dir < 1, a
 * NULL tape with T > 0, NULL t_r / t_y / t_r_out / t_y_out, det without t_taps or the reverse, n_det outside 1 .. n_cells with det:
 * DHTS_E_INVALID, nothing is dereferenced.
 * dhts_macro_jvp_plan: plan[0] 0 = general kernel, 1 = fast (2 <= n_cells <= 1024, T > 0)     plan[1] block size
 *   plan[2] direction slots of the widest launch (4, 2, 1; lanes too long for the general kernel's LDS at 4 directions take fewer)
 *   plan[3] number of launches (0 for T = 0)     plan[4 .. 7] 0.  n_det: 0 = no readings, else 1 .. n_cells.
 */
int dhts_macro_rollout_jvp(const dhts_macro_desc *d, int T, const float *tape, int n_dir,
                           const float *t_r, const float *t_y, const float *t_ghost, int ghost_is_sched,
                           float *t_r_out, float *t_y_out, const int32_t *det, int n_det, float *t_taps,
                           dhts_error *err, void *stream);
int dhts_macro_jvp_plan(const dhts_macro_desc *d, int T, int n_dir, int n_det, int32_t plan[8]);

/*
 * The rollout AND n_dir = K tangent directions of it in one kernel, without a tape: what dhts_macro_rollout_fwd (or _fwd_sched, or
 * _fwd_taps) followed by dhts_macro_rollout_jvp returns, bit for bit, from one entry point -- forward-mode differentiation of the
 * reference's lane rollout (road/lane/_macro_lane.py:83-146; the blocks are those of road/lane/dmacro_lane.py:96-132, applied
 * untransposed where :277-309 applies their transposes).  Forward mode walks the steps in the forward's order, so the interface products
 * of a step are used out of on-chip memory where the forward would store its tape entry: the tape (dhts_macro_tape_bytes) does not
 * exist, and no memory grows with T but the readings the caller asks for.  The arithmetic is the two calls' own (the same device
 * functions), in the same order; a direction's result does not depend on K, on its slot or on fused versus taped.
 *   r, y, u, ueq, ghost, ghost_is_sched, r_out .. ueq_out     as dhts_macro_rollout_fwd_taps: ghost [lane][2][4], or the schedule
 *                       [T][lane][2][4] with ghost_is_sched != 0.  The outputs must not alias the inputs (every launch reads them again).
 *   t_r, t_y, t_ghost, t_r_out, t_y_out     as dhts_macro_rollout_jvp, t_ghost following ghost_is_sched: NULL = zero,
 *                       [K][lane][2][2], or [K][T][lane][2][2] beside a schedule
 *   det, n_det, taps, t_taps     all three pointers or none: taps [T][lane][3][n_det] as dhts_macro_rollout_fwd_taps writes it, t_taps
 *                       [K][T][lane][2][n_det] as dhts_macro_rollout_jvp does.  The index contract is theirs: every det[j] is compared
 *                       against [0, n_cells) as an unsigned value before any address is formed from it; an entry outside writes nothing.
 * There is no state history (the taped operator has none either).  The kernel is the two-phase lane kernel's mapping (one workgroup per
 * lane; DHTS_OPT_MACRO_FWD_VARIANT and _GROUP do not apply), whose results the pair kernel equals bit for bit.  K directions run as
 * launches of 4, 2 or 1 (a remainder of 3 as one launch of 4 with a slot masked), at most the number dhts_macro_fwd_jvp_plan reports
 * per launch: 4 for lanes of up to 997 cells, 2 up to 1239, 1 up to 1410; a longer lane does not fit (its records, the interface
 * products and two tangent copies per direction exceed 160 KB of LDS) and keeps the taped pair.  Every launch recomputes the primal and
 * writes the same bits to r_out .. ueq_out; the first one alone writes taps and err.  T = 0: state and tangents come back as they went
 * in, no row of anything is addressed.
 * Two fault records, each nullable, kept apart as the pair keeps them:
 *   err       what the forward reports: DHTS_FAULT_CFL (step, lane, interface)
 *   err_jvp   what the tangent sweep reports: DHTS_FAULT_NAN with the lane's EARLIEST (step, cell) of a non-finite tangent
 * A bad descriptor, T < 0, n_dir < 1, a NULL r / y / u / ueq / ghost / t_r / t_y / r_out / y_out / u_out / ueq_out / t_r_out / t_y_out,
 * det without both taps and t_taps or the reverse, n_det outside 1 .. n_cells with det, or a lane that does not fit: DHTS_E_INVALID,
 * nothing is dereferenced.
 * dhts_macro_fwd_jvp_plan: plan[0] wavefronts per lane     plan[1] 64-cell passes per wavefront
 *   plan[2] direction slots of the widest launch (4, 2, 1; 0: the lane does not fit)     plan[3] number of launches (0 for T = 0 or
 *   when nothing fits)     plan[4] dynamic LDS bytes of the widest launch     plan[5 .. 7] 0.  n_det: 0 = no readings, else 1 .. n_cells.
 */
int dhts_macro_rollout_fwd_jvp(const dhts_macro_desc *d, int T, int n_dir,
                               const float *r, const float *y, const float *u, const float *ueq, const float *ghost, int ghost_is_sched,
                               const float *t_r, const float *t_y, const float *t_ghost,
                               float *r_out, float *y_out, float *u_out, float *ueq_out, float *t_r_out, float *t_y_out,
                               const int32_t *det, int n_det, float *taps, float *t_taps,
                               dhts_error *err, dhts_error *err_jvp, void *stream);
int dhts_macro_fwd_jvp_plan(const dhts_macro_desc *d, int T, int n_dir, int n_det, int32_t plan[8]);

/*
 * Reverse mode of the same rollout WITHOUT a tape in memory: what dhts_macro_rollout_fwd (or _fwd_sched, or _fwd_taps) followed by
 * dhts_macro_rollout_bwd (or _bwd_sched, or _bwd_taps) returns, bit for bit, from checkpoints.  Replaces the same T calls of
 * dMacroForwardLayer.forward / .backward (road/lane/_macro_lane.py:83-146, road/lane/dmacro_lane.py:96-132 and :277-309).
 * The forward keeps the float32 (r, y) every cell enters a step with each S steps (S = the segment); the reverse sweep runs a
 * segment again from its checkpoint with the forward's own step -- the same device functions on the same float32 operands, so the
 * interface products (A_i, B_i) are the taped forward's bits --, keeps them in on-chip memory for the S steps and sweeps them newest
 * first with the general reverse sweep's expressions, then moves to the checkpoint before.  Segment 0 is replayed from the call's
 * own inputs.
 *     ckpt    dhts_macro_ckpt_bytes = C x n_lanes x n_cells x 8 B, C = ceil(T / S) (0 for T = 0); opaque
 *             (the compact tape: dhts_macro_tape_bytes, about 46 B per cell and step)
 *   segment   0 = the plan's choice, else 1 .. the max_segment dhts_macro_ckpt_plan reports (the reverse kernel's LDS holds the
 *             products of a segment); the forward, the reverse sweep and dhts_macro_ckpt_bytes must be given the same value
 *   dhts_macro_rollout_fwd_ckpt   r, y, u, ueq, ghost, ghost_is_sched, r_out .. ueq_out, det, n_det, taps, err as
 *                                 dhts_macro_rollout_fwd_taps (same bits, DHTS_FAULT_CFL likewise), det and taps both NULL: no readings;
 *                                 ckpt is filled (NULL is accepted for T = 0).  There is no state history.
 *   dhts_macro_rollout_bwd_ckpt   r, y, u, ueq, ghost, ghost_is_sched: the forward's inputs (segment 0 and the boundary cells are read
 *                                 from them); g_r, g_y, det, n_det, g_taps, g_r_out, g_y_out, g_ghost, err as dhts_macro_rollout_bwd_taps
 *                                 (g_ghost [lane][2][2], or per step [T][lane][2][2] with ghost_is_sched; DHTS_FAULT_NAN likewise), det
 *                                 and g_taps both NULL: no per-step cotangents.  The replay reports no fault a second time.
 *                                 PRECONDITION: the entries of det inside [0, n_cells) are distinct.  This sweep adds ONE column of
 *                                 g_taps to a cell (the last that names it), dhts_macro_rollout_bwd_taps every one: with a repeated
 *                                 entry the two differ.  (dhts.macro_rollout checks a list of detectors; a device tensor it does not.)
 * Both kernels use the two-phase lane kernel's mapping (one workgroup per lane; DHTS_OPT_MACRO_FWD_WAVES, _VARIANT and _GROUP do not
 * apply).  A lane whose records, cotangent planes and ONE step of products exceed 160 KB of LDS (1320 cells and above) does not fit and
 * keeps the taped pair.  T = 0: the state resp. the cotangents come back as they went in (g_ghost [lane][2][2]: zeros), no row of
 * anything is addressed.
 * A bad descriptor, T < 0, a segment outside 0 .. max_segment, a lane that does not fit, a NULL r / y / u / ueq / ghost / r_out / y_out /
 * u_out / ueq_out resp. g_r / g_y / g_r_out / g_y_out (ckpt with T > 0; g_ghost with ghost_is_sched), det without taps resp. g_taps or
 * the reverse, n_det outside 1 .. n_cells with det: DHTS_E_INVALID, nothing is dereferenced (dhts_macro_ckpt_bytes: 0).
 * dhts_macro_ckpt_plan (n_det: 0 = no readings, else 1 .. n_cells; a pure function of its arguments, no device is needed):
 *   plan[0] wavefronts per lane     plan[1] 64-cell passes per wavefront     plan[2] the segment used (the plan's own for segment = 0)
 *   plan[3] max_segment (0: the lane does not fit; then only segment = 0 is answered, with plan[2], [4], [6], [7] = 0)
 *   plan[4] checkpoints C     plan[5] dynamic LDS bytes of the forward     plan[6] ... of the reverse kernel at that segment
 *   plan[7] reverse workgroups a CU holds by LDS
 */
int dhts_macro_ckpt_plan(const dhts_macro_desc *d, int T, int n_det, int segment, int32_t plan[8]);
size_t dhts_macro_ckpt_bytes(const dhts_macro_desc *d, int T, int segment);
int dhts_macro_rollout_fwd_ckpt(const dhts_macro_desc *d, int T, int segment,
                                const float *r, const float *y, const float *u, const float *ueq, const float *ghost, int ghost_is_sched,
                                float *r_out, float *y_out, float *u_out, float *ueq_out,
                                const int32_t *det, int n_det, float *taps, void *ckpt, dhts_error *err, void *stream);
int dhts_macro_rollout_bwd_ckpt(const dhts_macro_desc *d, int T, int segment, const void *ckpt,
                                const float *r, const float *y, const float *u, const float *ueq, const float *ghost, int ghost_is_sched,
                                const float *g_r, const float *g_y, const int32_t *det, int n_det, const float *g_taps,
                                float *g_r_out, float *g_y_out, double *g_ghost, dhts_error *err, void *stream);

/*
 * THE DENSE-FIT LOSS inside the checkpointed pair: sum((hist - observed)^2) over the density and the speed plane of the history and its
 * gradient, without hist and without g_hist.  The two entry points are dhts_macro_rollout_fwd_ckpt / _bwd_ckpt without det / n_det /
 * taps / g_taps, with
 *   target   [T][L][2][N] float32: target[t][l][0][k] = the observed density of cell k AFTER step t (what hist[t][l][0][k] holds),
 *            target[t][l][1][k] the observed speed (hist[t][l][2][k]).  A NaN entry is not observed: it adds exactly 0 to sse and no
 *            cotangent (NaN in the whole speed plane: a density-only fit).
 *   sse      [L][2] DOUBLE, written: per lane the sum over observed entries of the squared density residual, and of the squared speed
 *            residual.  The residual is the float32 difference x - target (what hist - observed is), squared and summed in double: each
 *            thread sums its own cells in step order, the wavefront combines its threads' sums pairwise (partners 32, 16 .. 1 apart) and
 *            thread 0 adds the wavefronts' sums in their order, through LDS.  No atomics: two runs give the same bits, and so do runs
 *            with different segments.  T = 0: 0.
 *   g_sse    [L][2] DOUBLE or NULL (zero: the sweep is then dhts_macro_rollout_bwd_ckpt's plain one): the cotangent of sse.  The
 *            cotangent of row t at cell k is gr = (float)(2 g_sse[l][0]) * (r - target_r), gy = 0, then the float32 glue of
 *            dhts_macro_u_tap_bwd with g_u = (float)(2 g_sse[l][1]) * (u - target_u) on the replayed (r, y) -- residual 0 for a NaN
 *            entry --, added where dhts_macro_rollout_bwd adds g_hist[t][l][:][k], with the same float32 add.
 *   r_fin, y_fin, u_fin   [L][N]: the forward's r_out, y_out, u_out = row T - 1 of the history, which the replay does not recompute;
 *            its cotangent goes into (g_r, g_y) in front of the sweep.  Needed with g_sse (T > 0).
 * and otherwise their siblings' arguments, arithmetic, fault records and bits (r_out .. ueq_out and, for equal per-step cotangents,
 * every gradient):
 *   dhts_macro_rollout_fwd_ckpt_target   the T calls of dMacroForwardLayer.forward (road/lane/_macro_lane.py:83-146,
 *       road/lane/dmacro_lane.py:96-132) and the loss of example/inverse/macro.py:34-68 on every cell and step.  ckpt may be NULL: no
 *       checkpoint is kept (a loss evaluation that nobody differentiates).
 *   dhts_macro_rollout_bwd_ckpt_target   the sweep of dMacroForwardLayer.backward (road/lane/dmacro_lane.py:277-309) with the loss's
 *       cotangent entering at every step.
 * target is read once per direction, coalesced along k; nothing of size T x N is written.
 * DHTS_E_INVALID, nothing dereferenced and nothing launched: whatever the siblings reject (but a NULL ckpt of the forward), a NULL sse,
 * a NULL target when T > 0, g_sse without r_fin / y_fin / u_fin when T > 0, a segment outside 0 .. the max_segment of
 * dhts_macro_ckpt_target_plan, a lane that plan does not fit.  T = 0: state and cotangents come back as they went in, sse = 0, no row
 * of anything is addressed.
 * dhts_macro_ckpt_target_plan: dhts_macro_ckpt_plan's eight entries for these two kernels (a pure function, no device).  The reverse
 * kernel's ring holds two more floats per cell-step (the finished cotangent pair: 32 (N + 1) + 8 N bytes a step), so max_segment and the
 * default segment (the same rule with that step size) are shorter, and the first lane that does not fit has 1240 cells (1320 for the
 * siblings); segment 0 at the two entry points is THIS plan's default.  The checkpoint buffer is dhts_macro_ckpt_bytes of the resolved
 * segment plan[2].
 */
int dhts_macro_ckpt_target_plan(const dhts_macro_desc *d, int T, int segment, int32_t plan[8]);
int dhts_macro_rollout_fwd_ckpt_target(const dhts_macro_desc *d, int T, int segment,
                                       const float *r, const float *y, const float *u, const float *ueq, const float *ghost, int ghost_is_sched,
                                       float *r_out, float *y_out, float *u_out, float *ueq_out, void *ckpt, const float *target, double *sse,
                                       dhts_error *err, void *stream);
int dhts_macro_rollout_bwd_ckpt_target(const dhts_macro_desc *d, int T, int segment, const void *ckpt,
                                       const float *r, const float *y, const float *u, const float *ueq, const float *ghost, int ghost_is_sched,
                                       const float *g_r, const float *g_y, const float *target, const double *g_sse, const float *r_fin,
                                       const float *y_fin, const float *u_fin, float *g_r_out, float *g_y_out, double *g_ghost,
                                       dhts_error *err, void *stream);
/* RING ROADS on the tape-free paths: the lane is closed, cell n_cells - 1 is the left neighbour of cell 0.  A ring lane has
 * n_cells >= 1 cells and the circumference n_cells dx: it takes no parameter.  In every step t the boundary record in front of cell 0
 * is a COPY of the record of cell n_cells - 1 as step t finds it -- (r, y, u, u_eq) and what the kernels derive from them, exactly
 * what cell k - 1 is to cell k -- and the one behind cell n_cells - 1 a copy of cell 0's; in step 0 these are the call's own inputs
 * of those cells.  Nothing else changes: same step, same float32 stores, same CFL rule, same fault records.  Interfaces 0 and n_cells
 * are the one seam: both are solved, from operands with equal bits, so their fluxes are equal bit for bit and the lane's mass
 * sum_k r[k] is conserved up to the float32 store of each cell.  (The record of a scheduled boundary cell is made from a float32 row,
 * the ring's copy is that of an interior cell: a ring agrees with a scheduled lane fed its own end cells within rounding, not in
 * every bit by contract.)
 *   n_cells = 1: the cell is its own neighbour on both sides and its state never changes.  n_cells = 2: each cell is the other's
 *   left and right neighbour.  T = 0: outputs, cotangents and tangents come back as they went in.
 * The five entry points are their siblings WITHOUT ghost, ghost_is_sched, g_ghost and t_ghost -- there is no boundary cell, hence no
 * cotangent and no tangent of one -- and with the siblings' other arguments, arithmetic, plans and DHTS_E_INVALID rules:
 *   dhts_macro_rollout_fwd_ckpt_ring          as dhts_macro_rollout_fwd_ckpt (det / n_det / taps or none).
 *   dhts_macro_rollout_bwd_ckpt_ring          as dhts_macro_rollout_bwd_ckpt.  The cotangent the sweep forms for the slot in front of
 *       cell 0 in a step goes to cell n_cells - 1, the one for the slot behind cell n_cells - 1 to cell 0, both in the same sweep step
 *       inside the hand-over (G + c2_left) + c0_right, whose order of additions is kept: for cell 0 the left term is that of cell
 *       n_cells - 1, for cell n_cells - 1 the right term is that of cell 0.
 *   dhts_macro_rollout_fwd_ckpt_target_ring / _bwd_ckpt_target_ring   the dense fit above on the ring (dhts_macro_ckpt_target_plan).
 *   dhts_macro_rollout_fwd_jvp_ring           as dhts_macro_rollout_fwd_jvp: the two boundary slots of the tangents a step reads hold
 *       the tangents of cells n_cells - 1 and 0.
 * dhts_macro_ckpt_plan, dhts_macro_ckpt_target_plan, dhts_macro_fwd_jvp_plan and dhts_macro_ckpt_bytes hold for the ring forms as
 * they stand (no LDS, no barrier and no global load is added), and so do the cell limits (1320 / 1240 / 1410).
 * DHTS_FAULT_CFL at the seam: interfaces 0 and n_cells fail together; the record names interface 0 (the kernels record a fault of
 * interface n_cells as one of interface 0: on a ring they are the same interface), with the step and lane as on an open lane. */
int dhts_macro_rollout_fwd_ckpt_ring(const dhts_macro_desc *d, int T, int segment,
                                     const float *r, const float *y, const float *u, const float *ueq,
                                     float *r_out, float *y_out, float *u_out, float *ueq_out,
                                     const int32_t *det, int n_det, float *taps, void *ckpt, dhts_error *err, void *stream);
int dhts_macro_rollout_bwd_ckpt_ring(const dhts_macro_desc *d, int T, int segment, const void *ckpt,
                                     const float *r, const float *y, const float *u, const float *ueq,
                                     const float *g_r, const float *g_y, const int32_t *det, int n_det, const float *g_taps,
                                     float *g_r_out, float *g_y_out, dhts_error *err, void *stream);
int dhts_macro_rollout_fwd_ckpt_target_ring(const dhts_macro_desc *d, int T, int segment,
                                            const float *r, const float *y, const float *u, const float *ueq,
                                            float *r_out, float *y_out, float *u_out, float *ueq_out, void *ckpt, const float *target,
                                            double *sse, dhts_error *err, void *stream);
int dhts_macro_rollout_bwd_ckpt_target_ring(const dhts_macro_desc *d, int T, int segment, const void *ckpt,
                                            const float *r, const float *y, const float *u, const float *ueq,
                                            const float *g_r, const float *g_y, const float *target, const double *g_sse, const float *r_fin,
                                            const float *y_fin, const float *u_fin, float *g_r_out, float *g_y_out,
                                            dhts_error *err, void *stream);
int dhts_macro_rollout_fwd_jvp_ring(const dhts_macro_desc *d, int T, int n_dir,
                                    const float *r, const float *y, const float *u, const float *ueq, const float *t_r, const float *t_y,
                                    float *r_out, float *y_out, float *u_out, float *ueq_out, float *t_r_out, float *t_y_out,
                                    const int32_t *det, int n_det, float *taps, float *t_taps,
                                    dhts_error *err, dhts_error *err_jvp, void *stream);
/* ---- on-ramp inflow at chosen cells of the checkpointed pair ----
 * A source term in chosen cells: ramps [n_ramp] are cell indices shared by all lanes, inflow [T][n_lanes][n_ramp] float32 the density
 * rate (normalised density per second) that cell ramps[j] of lane l gets in step t.  Behind the Godunov update of step t, whose
 * float32 store is unchanged, the owner of a ramp cell forms
 *     r' = (float)((double)r + dt * (double)inflow[t][l][j]),   y' = y,
 * and (u, u_eq) of the cell are the step's glue of (r', y): two roundings, the step's own and the source's.  Everything that reads
 * "the state after step t" -- the next step, a ring's copies of its end cells, the checkpoint rows, the readings, the residual against
 * `target`, the outputs -- sees (r', y).  A negative entry is an off-ramp; nothing is clamped and no fault code is added: keeping r
 * inside (0, 1) is the caller's business, and DHTS_FAULT_CFL still catches a runaway.
 * Reverse: the source is identity in (r, y), so the sweep is the siblings' and
 *     g_inflow[t][l][j] = (float)(dt * (double)G_r),
 * G_r the cotangent of r at cell ramps[j] of the state after step t, that row's detector column or target pair included (row T - 1:
 * of the incoming cotangent).  g_inflow [T][n_lanes][n_ramp] float32: every entry is written.
 *   dhts_macro_rollout_fwd_ckpt_ramp          as dhts_macro_rollout_fwd_ckpt        (ring: as dhts_macro_rollout_fwd_ckpt_ring)
 *   dhts_macro_rollout_bwd_ckpt_ramp          as dhts_macro_rollout_bwd_ckpt        (ring: as dhts_macro_rollout_bwd_ckpt_ring)
 *   dhts_macro_rollout_fwd_ckpt_target_ramp   as dhts_macro_rollout_fwd_ckpt_target (ring: as ..._fwd_ckpt_target_ring)
 *   dhts_macro_rollout_bwd_ckpt_target_ramp   as dhts_macro_rollout_bwd_ckpt_target (ring: as ..._bwd_ckpt_target_ring)
 * with the siblings' arguments, plans (dhts_macro_ckpt_plan resp. dhts_macro_ckpt_target_plan, dhts_macro_ckpt_bytes: no LDS is added),
 * arithmetic and DHTS_E_INVALID rules, plus ramps / n_ramp / inflow (reverse: and g_inflow) and `ring`: nonzero = the lane is closed,
 * `ghost` must be NULL, ghost_is_sched is not read and g_ghost is not written.
 * DHTS_E_INVALID besides: n_ramp outside 1 .. n_cells; with T > 0 a NULL ramps or inflow, reverse also a NULL g_inflow; ring with a
 * ghost.  Nothing is dereferenced or launched then.  T = 0: state and cotangents come back as they went in, no row is addressed.
 * An index of ramps outside [0, n_cells) names no cell: nothing is added for it, no address is formed from it, and its column of
 * g_inflow is 0.  PRECONDITION (as for det of the reverse sweep): the entries of ramps inside [0, n_cells) are distinct; with a
 * repeated entry one of its columns is used and the result is unspecified, but memory-safe. */
int dhts_macro_rollout_fwd_ckpt_ramp(const dhts_macro_desc *d, int T, int segment,
                                     const float *r, const float *y, const float *u, const float *ueq, const float *ghost, int ghost_is_sched,
                                     float *r_out, float *y_out, float *u_out, float *ueq_out,
                                     const int32_t *det, int n_det, float *taps, void *ckpt,
                                     const int32_t *ramps, int n_ramp, const float *inflow, int ring, dhts_error *err, void *stream);
int dhts_macro_rollout_bwd_ckpt_ramp(const dhts_macro_desc *d, int T, int segment, const void *ckpt,
                                     const float *r, const float *y, const float *u, const float *ueq, const float *ghost, int ghost_is_sched,
                                     const float *g_r, const float *g_y, const int32_t *det, int n_det, const float *g_taps,
                                     float *g_r_out, float *g_y_out, double *g_ghost,
                                     const int32_t *ramps, int n_ramp, const float *inflow, float *g_inflow, int ring, dhts_error *err,
                                     void *stream);
int dhts_macro_rollout_fwd_ckpt_target_ramp(const dhts_macro_desc *d, int T, int segment,
                                            const float *r, const float *y, const float *u, const float *ueq, const float *ghost,
                                            int ghost_is_sched, float *r_out, float *y_out, float *u_out, float *ueq_out, void *ckpt,
                                            const float *target, double *sse,
                                            const int32_t *ramps, int n_ramp, const float *inflow, int ring, dhts_error *err, void *stream);
int dhts_macro_rollout_bwd_ckpt_target_ramp(const dhts_macro_desc *d, int T, int segment, const void *ckpt,
                                            const float *r, const float *y, const float *u, const float *ueq, const float *ghost,
                                            int ghost_is_sched, const float *g_r, const float *g_y, const float *target, const double *g_sse,
                                            const float *r_fin, const float *y_fin, const float *u_fin, float *g_r_out, float *g_y_out,
                                            double *g_ghost, const int32_t *ramps, int n_ramp, const float *inflow, float *g_inflow, int ring,
                                            dhts_error *err, void *stream);
/* ---- on-ramp inflow and its tangent on the fused forward + tangent kernel ----
 * The source above in forward mode, without a tape: the T calls of dMacroForwardLayer.forward (road/lane/_macro_lane.py:83-146, the
 * blocks of road/lane/dmacro_lane.py:96-132 applied untransposed, :126-129) with the source of the _ckpt_ramp entry points behind every
 * step and its tangent behind the step's tangent.  ramps [n_ramp], inflow [T][n_lanes][n_ramp] as there; t_inflow
 * [n_dir][T][n_lanes][n_ramp] float32 the tangent of inflow per direction, or NULL: zero (nothing is read).  Behind the Godunov
 * update of step t the owner of cell ramps[j] forms r' = (float)((double)r + dt * (double)inflow[t][l][j]), y' = y, as the
 * checkpointed forward does -- the primal outputs and readings are dhts_macro_rollout_fwd_ckpt_ramp's bits -- and behind the cell's
 * tangent step, for every direction d,
 *     t_r' = (float)((double)t_r + dt * (double)t_inflow[d][t][l][j]),   t_y' = t_y.
 * Everything that reads the state or the tangents after step t -- the next step, a ring's copies of its end cells, the finiteness
 * test of err_jvp, the readings and their tangents, the outputs -- sees the primed values.
 *   dhts_macro_rollout_fwd_jvp_ramp        as dhts_macro_rollout_fwd_jvp (constant or scheduled boundary cells, ghost_is_sched)
 *   dhts_macro_rollout_fwd_jvp_ring_ramp   as dhts_macro_rollout_fwd_jvp_ring
 * with the siblings' arguments in the siblings' order, then ramps, n_ramp, inflow, t_inflow; the siblings' arithmetic, fault
 * records, DHTS_E_INVALID rules and plan (dhts_macro_fwd_jvp_plan and the cell limits 997 / 1239 / 1410 hold as they stand: no LDS,
 * no barrier and no atomic is added).  Every launch of a call recomputes the primal with the source; launches after the first read the
 * same inflow and their own directions of t_inflow.  n_ramp = 0: the sibling's call, the three arrays are not read.
 * DHTS_E_INVALID besides, nothing dereferenced and nothing launched: n_ramp < 0; n_ramp > 0 with T > 0 and a NULL ramps or inflow.
 * T = 0: state and tangents come back as they went in, no row is addressed.  An index of ramps outside [0, n_cells) names no cell:
 * nothing is added for it and no address is formed from it.  PRECONDITION as above: the entries inside [0, n_cells) are distinct. */
int dhts_macro_rollout_fwd_jvp_ramp(const dhts_macro_desc *d, int T, int n_dir,
                                    const float *r, const float *y, const float *u, const float *ueq, const float *ghost, int ghost_is_sched,
                                    const float *t_r, const float *t_y, const float *t_ghost,
                                    float *r_out, float *y_out, float *u_out, float *ueq_out, float *t_r_out, float *t_y_out,
                                    const int32_t *det, int n_det, float *taps, float *t_taps,
                                    dhts_error *err, dhts_error *err_jvp, void *stream,
                                    const int32_t *ramps, int n_ramp, const float *inflow, const float *t_inflow);
int dhts_macro_rollout_fwd_jvp_ring_ramp(const dhts_macro_desc *d, int T, int n_dir,
                                         const float *r, const float *y, const float *u, const float *ueq, const float *t_r, const float *t_y,
                                         float *r_out, float *y_out, float *u_out, float *ueq_out, float *t_r_out, float *t_y_out,
                                         const int32_t *det, int n_det, float *taps, float *t_taps,
                                         dhts_error *err, dhts_error *err_jvp, void *stream,
                                         const int32_t *ramps, int n_ramp, const float *inflow, const float *t_inflow);
/* tangent of y = r (u - u_eq(r)): t_y = (dy/dr) t_r + (dy/du) t_u, the partials dhts_macro_state_from_ru_bwd applies, in float32 */
int dhts_macro_state_from_ru_jvp(int64_t n, double u_max, const float *r, const float *u, const float *t_r, const float *t_u,
                                 float *t_y, void *stream);
/* tangent of the speed tap: t_u = (du/dr) t_r + (du/dy) t_y, the partials of dhts_macro_u_tap_bwd (below eps the density is a constant) */
int dhts_macro_u_tap_jvp(int64_t n, double u_max, const float *r, const float *y, const float *t_r, const float *t_y,
                         float *t_u, void *stream);

/* One step = the drop-in for a batch of dMacroForwardLayer.forward / .backward calls (T = 1 of the above;
 * tape is one step's worth).
 * A ghost cell of Python floats: the reference's Riemann solve reads a boundary cell that holds plain floats in double
 * (dMacroLane.decell leaves them alone); the one such cell of the itscp networks is a SOURCE lane's upstream ghost (_simulator.py:68-71:
 * r = the inflow of the schedule, u = u_eq(r), hence y = 0).  The step operator takes it as the LEFT quad {NaN, 0, low 32 bits of the
 * double r, high 32 bits} (bit patterns in the float slots; csrc/arz_device.hpp::ghost_source_pack): a NaN density marks it, u = u_eq(r)
 * is evaluated in double.  dhts_net_ghosts_fwd writes source lanes that way; the cotangent of such a ghost is of no use.  (The T-step
 * rollouts of straight lanes above take float32 ghosts only.) */
int dhts_macro_step_fwd(const dhts_macro_desc *d,
                        const float *r, const float *y, const float *u, const float *ueq, const float *ghost,
                        float *r_out, float *y_out, float *u_out, float *ueq_out,
                        float *tape, dhts_error *err, void *stream);
int dhts_macro_step_bwd(const dhts_macro_desc *d, const float *tape, const float *g_r, const float *g_y,
                        float *g_r_out, float *g_y_out, double *g_ghost, dhts_error *err, void *stream);

/* ---- micro (IDM) ------------------------------------------------------------------------------- */
typedef struct dhts_micro_desc {
    int32_t n_lanes;   /* L */
    int32_t capacity;  /* V: vehicle slots per lane (1 .. DHTS_MICRO_MAX_VEHICLES); slot i follows slot i+1,
                          head = slot count-1 (MicroLane.curr_vehicle order, _micro_lane.py:31-34) */
    double dt;
} dhts_micro_desc;

#define DHTS_MICRO_MAX_VEHICLES 1024
#define DHTS_MICRO_NPARAM 6 /* accel_max, accel_pref, target_speed, min_space, time_pref, length (micro_vehicle.py:21-28) */

/* bytes of Jacobian tape for T fused steps (dhts_micro_rollout_*): [step][lane][Vp][3] float32 = (dEgo[1][0], dEgo[1][1],
 * dLeading[1][1]) of every vehicle (12 B per vehicle-step).  The first rows of both blocks are the constants [1, dt] and
 * [0, 0], and dLeading[1][0] = -dEgo[1][0] bit for bit (didm.py:38-103); the reverse sweep re-inserts them, so results equal
 * those of the 32-byte dqs[a][2][2][2] tape */
size_t dhts_micro_tape_bytes(const dhts_micro_desc *d, int T);
/* bytes of the single-step operator's tape (dhts_micro_step_*): [lane][2][Vp][4] float32, plane k = dqs[a][k] */
size_t dhts_micro_step_tape_bytes(const dhts_micro_desc *d);

/*
 * n independent vehicles: IDM.compute_acceleration (model/micro/_idm.py:6-50) + one explicit-Euler step
 * (_micro_lane.py:182-183) + dIDM.compute_dEgo / compute_dLeading (model/micro/didm.py:13-103).
 *   variant 0 = production arithmetic, 1 = reference-order IEEE division / square root
 *   in  [9][n] DOUBLE (SoA): a_max a_pref v v_target position_delta speed_delta min_space time_pref delta_time
 *   out next_pv [2][n] DOUBLE: (0 + dt v, v + dt acc) rounded to float32; dEgo, dLeading [4][n] float32;
 *       collided [n] int32 (position_delta < 0); acc_sstar [2][n] DOUBLE = (acceleration, clipped optimal spacing);
 *       clips [2][n] int32 = (clipped_acceleration, clipped_optimal_spacing)
 */
int dhts_idm_batch(int64_t n, int variant, const double *in, double *next_pv, float *dEgo, float *dLeading, int32_t *collided,
                   double *acc_sstar, int32_t *clips, void *stream);

/* The Jacobians alone, from the caller's optimal spacing and clip flags: dIDM.compute_dEgo / compute_dLeading as the reference
 * declares them (model/micro/didm.py:13-103; dMicroLane._backward passes the flags of the forward pass -- derived from the gap
 * clamped to 1e-5 -- beside the UN-clamped gap, dmicro_lane.py:97).
 *   in  [12][n] DOUBLE (SoA): a_max a_pref v v_target position_delta speed_delta min_space time_pref optimal_spacing delta_time
 *       clipped_acceleration clipped_optimal_spacing (0 / 1)
 *   out dEgo, dLeading [4][n] float32 */
int dhts_idm_jac_batch(int64_t n, const double *in, float *dEgo, float *dLeading, void *stream);

/*
 * T fused steps of L independent lanes: replaces T x L calls of dMicroForwardLayer.forward
 * (dmicro_lane.py:230-269 = MicroLane.forward _micro_lane.py:131-214 + dMicroLane._backward :87-127).
 *   in : p, v [L][V]; count [L] int32 vehicles per lane or NULL (= V everywhere);
 *        params [6][L][V] DOUBLE (the reference keeps them as Python floats);
 *        head [L][2] DOUBLE = (head_position_delta, head_speed_delta) per lane, constant over the rollout
 *        (defaults 1000 / 0, _micro_lane.py:14-15)
 *   out: p_out, v_out [L][V]; tape or NULL; hist [T][L][2][V] = (p, v) after every step, or NULL
 */
int dhts_micro_rollout_fwd(const dhts_micro_desc *d, int T,
                           const float *p, const float *v, const int32_t *count, const double *params, const double *head,
                           float *p_out, float *v_out, float *tape, float *hist, dhts_error *err, void *stream);
/*
 * Reverse sweep: replaces T x L calls of dMicroForwardLayer.backward (dmicro_lane.py:271-298), including the
 * virtual-leader slot of dMicroLane.vectorize_input (:130-153) whose cotangent returns to the head vehicle and
 * to (head_position_delta, head_speed_delta).
 *   in : g_p, g_v [L][V]; g_hist [T][L][2][V] optional
 *   out: g_p_out, g_v_out [L][V]; g_head [L][2] DOUBLE = cotangent of (head_position_delta, head_speed_delta)
 */
int dhts_micro_rollout_bwd(const dhts_micro_desc *d, int T, const float *tape, const int32_t *count,
                           const float *g_p, const float *g_v, const float *g_hist,
                           float *g_p_out, float *g_v_out, double *g_head, dhts_error *err, void *stream);

/*
 * The same rollout, differentiated with respect to the DRIVER PARAMETERS as well: what autograd of the reference's plain MicroLane
 * (road/lane/_micro_lane.py:131-214 over IDM.compute_acceleration, model/micro/_idm.py:30-49) gives when the attributes of its
 * MicroVehicles are tensors -- the derivative of every step as the forward executed it, summed over the steps.  With gv = the cotangent
 * of a vehicle's speed after a step (g_hist term included) a step adds gv dt d acc / d theta to the vehicle's own parameters:
 *     c = v dv / (2 sqrt(a b))     s = max(s0 + v T + c, 0)     F = 1 - (v / v0)^4 - (s / gap)^2     Q = -2 a s / gap^2
 *     d/da = F - Q c / (2 a)    d/db = -Q c / (2 b)    d/dv0 = 4 a (v / v0)^4 / v0    d/ds0 = Q    d/dT = Q v
 * (spacing clip: the Q terms vanish; acceleration clip: nothing), and, through gap = |p_lead - p| - (len_lead + len) / 2 (:211),
 * -0.5 gv dt (2 a s^2 / gap^3) to the vehicle's own length and to its leader's -- not for the head vehicle (its gap is
 * head_position_delta) nor where the forward replaced the gap by a constant (collision :151-160, POSITION_DELTA_EPS :166).
 *
 * dhts_micro_rollout_fwd_params computes, and writes to p_out / v_out / tape / hist, exactly what dhts_micro_rollout_fwd does, and
 * fills the PARAMETER TAPE ptape beside it (tape and ptape are both required).  ptape is opaque; dhts_micro_param_tape_bytes sizes it:
 *     64 B header (names the shape it was written for) | head gaps [L][2] double, rounded up to whole 64 B |
 *     [step][lane][Vp] x 8 B = the float32 (p, v) the vehicle entered the step with        (Vp = capacity rounded up to 64)
 * i.e. 8 bytes per vehicle-step beside the tape's 12: the reverse sweep recomputes the partials in double from that state, the
 * leader's and params; the acceleration clip is the forward's own decision, read off the tape entry.
 * dhts_micro_rollout_bwd_params is dhts_micro_rollout_bwd (same g_p_out, g_v_out, g_head, bit for bit) and returns
 *     g_params [6][L][V] DOUBLE, laid out like params (slots at or beyond a lane's count: 0)
 * summed per vehicle in double, in step order, without atomics (bitwise repeatable).  params must be the forward's.  A ptape that
 * was written for another shape is not read: DHTS_FAULT_CAPACITY (index -3) and g_params = NaN.
 */
size_t dhts_micro_param_tape_bytes(const dhts_micro_desc *d, int T);
int dhts_micro_rollout_fwd_params(const dhts_micro_desc *d, int T,
                                  const float *p, const float *v, const int32_t *count, const double *params, const double *head,
                                  float *p_out, float *v_out, float *tape, void *ptape, float *hist, dhts_error *err, void *stream);
int dhts_micro_rollout_bwd_params(const dhts_micro_desc *d, int T, const float *tape, const void *ptape, const int32_t *count,
                                  const double *params, const float *g_p, const float *g_v, const float *g_hist,
                                  float *g_p_out, float *g_v_out, double *g_head, double *g_params, dhts_error *err, void *stream);
/* The parameter partials alone, n independent operand sets (the function the reverse sweep above calls):
 *   in    [9][n] DOUBLE (SoA) as dhts_idm_batch: a_max a_pref v v_target position_delta speed_delta min_space time_pref delta_time,
 *         position_delta RAW: the collision rule and the clamp to 1e-5 (_micro_lane.py:151-166) are applied here
 *   out   dacc [6][n] DOUBLE = d acc / d (a_max, a_pref, v_target, min_space, time_pref, position_delta), the last one 0 where the
 *         gap was replaced by a constant, all 0 under the acceleration clip; clips [2][n] int32 = (clipped_acceleration,
 *         clipped_optimal_spacing) as this step derived them */
int dhts_idm_param_jac_batch(int64_t n, const double *in, double *dacc, int32_t *clips, void *stream);

/* Which kernel instantiations the calls above launch (see dhts_macro_rollout_plan):
 *   plan[0] forward wavefronts per lane (1, 2, 4)     plan[1] passes per thread (the literal K: 1, 2, 4, 8, 16)
 *   plan[2] 1 = the full-lane instantiation (count == NULL and capacity = 64 x wavefronts x passes)
 *   plan[3] reverse sweep: 1 = the prefetched one-vehicle-per-thread path, 0 = the strided loop     plan[4] its block size
 *   plan[5] the parameter tape's bytes per vehicle-step (8 = pre-step state, partials recomputed by the reverse sweep)
 *   plan[6] block size of dhts_micro_rollout_bwd_params (the whole lane: always one vehicle per thread) */
int dhts_micro_rollout_plan(const dhts_micro_desc *d, int T, int has_count, int32_t plan[8]);

/*
 * Forward-mode tangent sweep (Jacobian-vector products) over a rollout's tape: n_dir = K directions in one call, oldest step first --
 * what forward-mode autograd of the reference's plain MicroLane rollout gives (road/lane/_micro_lane.py:131-214 over
 * IDM.compute_acceleration, model/micro/_idm.py:30-49), as dhts_micro_rollout_bwd / _bwd_params are its reverse mode.  The sweep
 * applies the blocks the reverse sweep applies transposed, dEgo = [[1, dt], [e2, e3]] and dLeading = [[0, 0], [-e2, l3]] of the tape
 * entry (e2, e3, l3), every 2-term product a float32 multiply + fused multiply-add; (t_pl, t_vl) = the leader's tangents before the step:
 *     t_p' = 1 t_p + dt t_v          t_v' = ((e2 t_p + e3 t_v) + (-e2 t_pl + l3 t_vl)) + x
 * The head vehicle (slot count - 1) follows the virtual leader (p + head_dp, v - head_dv), the reverse sweep's sign convention:
 *     t_pl = (float)((double)t_p + t_head[0])        t_vl = (float)((double)t_v - t_head[1])
 * x = +0.f without t_params.  With t_params (then ptape = the parameter tape of dhts_micro_rollout_fwd_params and params = the forward's
 * are required too; the three go together) x = (float)(dt c), c summed in double with fused multiply-adds in this order:
 *     c = sum_{q = 0 .. 4} (d acc / d theta_q) t_theta_q  [+ (d acc / d gap) (-(t_len_leader + t_len) / 2)  where the gap is live]
 * the partials those of dhts_micro_rollout_bwd_params (dhts_idm_param_jac_batch), recomputed from ptape's pre-step state; under the
 * acceleration clip (tape entry all zero) x = +0.f.  A direction's result does not depend on K or on its place among the directions, bit
 * for bit; t_params = 0 gives the bits of the call without it.
 *   tape                the rollout's tape (dhts_micro_tape_bytes); NULL is accepted for T = 0
 *   t_p, t_v            [K][lane][V] float32: tangent of the initial (p, v)      t_p_out, t_v_out: of the final one
 *   t_head              [K][lane][2] DOUBLE: tangent of (head_position_delta, head_speed_delta), or NULL (zero)
 *   t_params            [K][6][lane][V] DOUBLE, laid out like params per direction, or NULL
 *   t_hist              [K][T][lane][2][V] float32 or NULL: the tangent of what hist holds after every step
 * Slots at or beyond a lane's count return exactly 0 (in t_hist too), as the reverse sweep does: the two sweeps are adjoint.
 * K directions run as launches of 4, 2 or 1 (a remainder of 3 as one launch of 4 with a slot masked); with t_params a launch carries at
 * most the number dhts_micro_jvp_plan reports.  err: the lane's earliest non-finite tangent raises DHTS_FAULT_NAN (step, lane, vehicle);
 * a ptape that was written for another shape is not read beyond its header: DHTS_FAULT_CAPACITY (index -3), tangents = NaN.
 * A bad descriptor, T < 0, n_dir < 1, a NULL tape with T > 0, NULL t_p / t_v / t_p_out / t_v_out, or ptape / params / t_params not all
 * three or none: DHTS_E_INVALID, nothing is dereferenced.
 * dhts_micro_jvp_plan: plan[0] block size (the lane rounded up to 64: one vehicle per thread)
 *   plan[1] direction slots of the widest launch     plan[2] number of launches     plan[3] its dynamic LDS bytes     plan[4 .. 7] 0
 */
int dhts_micro_rollout_jvp(const dhts_micro_desc *d, int T, int n_dir, const float *tape, const void *ptape, const int32_t *count,
                           const double *params, const float *t_p, const float *t_v, const double *t_head, const double *t_params,
                           float *t_p_out, float *t_v_out, float *t_hist, dhts_error *err, void *stream);
int dhts_micro_jvp_plan(const dhts_micro_desc *d, int T, int n_dir, int want_params, int32_t plan[8]);

/*
 * The rollout AND n_dir = K tangent directions of it in one kernel, without a tape: what dhts_micro_rollout_fwd (or _fwd_params, with
 * t_params) followed by dhts_micro_rollout_jvp returns, bit for bit, from one entry point -- forward-mode autograd of the reference's
 * plain MicroLane rollout (road/lane/_micro_lane.py:131-214 over IDM.compute_acceleration, model/micro/_idm.py:30-49; the blocks are
 * those of road/lane/dmicro_lane.py:87-127).  Forward mode walks the steps in the forward's order, so a step's blocks (e2, e3, l3) and
 * the pre-step (p, v) the parameter partials are recomputed from are used out of the forward's registers: neither the tape
 * (dhts_micro_tape_bytes) nor the parameter tape (dhts_micro_param_tape_bytes) exists, and no memory grows with T unless hist / t_hist
 * are asked for.  The arithmetic is the two calls' own (the same device functions), in the same order.
 *   p, v, count, params, head, p_out, v_out, hist     as dhts_micro_rollout_fwd (slots at or beyond count pass through; hist or NULL)
 *   t_p, t_v, t_head, t_params, t_p_out, t_v_out, t_hist     as dhts_micro_rollout_jvp (slots at or beyond count exactly 0)
 * A non-NULL t_params selects the instantiation that carries the parameter term.  K directions run as launches of 4, 2 or 1 (a
 * remainder of 3 as one launch of 4 with a slot masked), at most the number dhts_micro_fwd_jvp_plan reports per launch; every launch
 * recomputes the primal and writes the same bits to p_out, v_out, the first one alone writes hist.  T = 0 launches too (it copies the
 * state and the live tangents and zeroes the rest).
 * Two fault records, each nullable, because the two checks of the pair do not collapse into one first-wins word:
 *   err       what the forward reports: DHTS_FAULT_COLLISION (step, lane, vehicle) -- printed and tolerated by the reference
 *   err_jvp   what the tangent sweep reports: DHTS_FAULT_NAN with the lane's EARLIEST (step, vehicle) of a non-finite tangent
 * A bad descriptor, T < 0, n_dir < 1, or a NULL p / v / params / head / t_p / t_v / p_out / v_out / t_p_out / t_v_out: DHTS_E_INVALID,
 * nothing is dereferenced.
 * dhts_micro_fwd_jvp_plan: plan[0] block size (the lane rounded up to 64: one vehicle per thread)
 *   plan[1] direction slots of the widest launch     plan[2] number of launches     plan[3] its dynamic LDS bytes     plan[4 .. 7] 0
 */
int dhts_micro_rollout_fwd_jvp(const dhts_micro_desc *d, int T, int n_dir, const float *p, const float *v, const int32_t *count,
                               const double *params, const double *head, const float *t_p, const float *t_v, const double *t_head,
                               const double *t_params, float *p_out, float *v_out, float *t_p_out, float *t_v_out, float *hist,
                               float *t_hist, dhts_error *err, dhts_error *err_jvp, void *stream);
int dhts_micro_fwd_jvp_plan(const dhts_micro_desc *d, int T, int n_dir, int want_params, int32_t plan[8]);

/*
 * The rollout's REVERSE mode without a tape in memory: what dhts_micro_rollout_fwd + dhts_micro_rollout_bwd (or _fwd_params +
 * _bwd_params, with g_params) return, bit for bit, from checkpoints.  Replaces the same T x L calls of dMicroForwardLayer.forward
 * (dmicro_lane.py:230-269 = MicroLane.forward _micro_lane.py:131-214 + dMicroLane._backward :87-127) and of
 * dMicroForwardLayer.backward (dmicro_lane.py:271-298, with the virtual-leader slot of dMicroLane.vectorize_input :130-153); the
 * parameter gradient is that of road/lane/_micro_lane.py:131-214 over IDM.compute_acceleration, model/micro/_idm.py:30-49.
 * The forward keeps the float32 state every S steps (S = the segment); the reverse sweep takes the segments last to first: it steps a
 * segment again from its checkpoint -- the same device function on the same float32 operands, so the entries (e2, e3, l3) and the
 * pre-step (p, v) are the tapes' bits --, holds them in LDS, and sweeps them newest first.  Neither the tape (dhts_micro_tape_bytes)
 * nor the parameter tape (dhts_micro_param_tape_bytes) exists; what grows with T is
 *     ckpt    dhts_micro_ckpt_bytes = C x L x Vp x 8 B, C = ceil(T / S) (0 for T = 0), Vp = capacity rounded up to 64; opaque
 * i.e. 8 B per vehicle per S steps instead of 12 B (20 B with the parameter tape) per vehicle-step.
 *   segment   0 = the plan's choice, else 1 .. the max_segment dhts_micro_ckpt_plan reports (the reverse kernel's LDS holds a segment:
 *             fewer steps with g_params); the forward, the reverse sweep and dhts_micro_ckpt_bytes must be given the same value
 *   dhts_micro_rollout_fwd_ckpt   p, v, count, params, head, p_out, v_out, hist, err as dhts_micro_rollout_fwd (same bits, hist at live
 *                                 slots; DHTS_FAULT_COLLISION likewise); ckpt is filled (NULL is accepted for T = 0)
 *   dhts_micro_rollout_bwd_ckpt   count, params, head: the forward's; g_p, g_v, g_hist, g_p_out, g_v_out, g_head, err as
 *                                 dhts_micro_rollout_bwd; g_params [6][L][V] DOUBLE as dhts_micro_rollout_bwd_params, or NULL: state only
 * The replay raises no collision again.  err of the reverse sweep: DHTS_FAULT_NAN at the latest step, lowest vehicle, as the taped sweep.
 * A bad descriptor, T < 0, a segment outside 0 .. max_segment, or a NULL p / v / params / head / p_out / v_out / g_p / g_v / g_p_out /
 * g_v_out (ckpt with T > 0): DHTS_E_INVALID, nothing is dereferenced (dhts_micro_ckpt_bytes: 0).
 * dhts_micro_ckpt_plan (want_params: the reverse sweep will be handed g_params):
 *   plan[0] block size of both kernels (the lane rounded up to 64: one vehicle per thread)     plan[1] the segment S used
 *   plan[2] max_segment     plan[3] C     plan[4] dynamic LDS bytes of the forward     plan[5] of the reverse kernel
 *   plan[6] reverse workgroups a CU holds by LDS (160 KB / plan[5])     plan[7] 0
 */
int dhts_micro_ckpt_plan(const dhts_micro_desc *d, int T, int want_params, int segment, int32_t plan[8]);
size_t dhts_micro_ckpt_bytes(const dhts_micro_desc *d, int T, int segment);
int dhts_micro_rollout_fwd_ckpt(const dhts_micro_desc *d, int T, int segment, const float *p, const float *v, const int32_t *count,
                                const double *params, const double *head, float *p_out, float *v_out, void *ckpt, float *hist,
                                dhts_error *err, void *stream);
int dhts_micro_rollout_bwd_ckpt(const dhts_micro_desc *d, int T, int segment, const void *ckpt, const int32_t *count, const double *params,
                                const double *head, const float *g_p, const float *g_v, const float *g_hist, float *g_p_out,
                                float *g_v_out, double *g_head, double *g_params, dhts_error *err, void *stream);

/*
 * PROBE SAMPLES on the two tape-free paths: the trajectory of a few vehicle slots every so many steps, read, written and
 * differentiated without a [T][L][2][V] history.  The three entry points are dhts_micro_rollout_fwd_ckpt, _bwd_ckpt and _fwd_jvp with
 * hist / g_hist / t_hist replaced by
 *   probes      [n_probes] int32 device, DISTINCT slots: column i of a row belongs to slot probes[i]; or NULL: every slot, column i =
 *               slot i (n_probes is ignored, P = capacity).  An entry outside [0, capacity) is skipped: no address is formed from it
 *               and its column is neither written nor read.  With a repeated entry only one of its columns is served.
 *   n_probes    P = 1 .. capacity with a list
 *   every       E >= 1: row j holds the state after step (j + 1) E - 1; the trailing T mod E steps have no row
 *   samples / g_samples   [T / E][L][2][P] float32, (p, v) as hist holds them; t_samples [K][T / E][L][2][P]
 * and otherwise their siblings' arguments, arithmetic, fault records and bits.
 *   dhts_micro_rollout_fwd_ckpt_samples   the rollout of dMicroForwardLayer.forward (dmicro_lane.py:230-269 = MicroLane.forward
 *       _micro_lane.py:131-214 + dMicroLane._backward :87-127), as dhts_micro_rollout_fwd_ckpt.  samples: written at live probe slots
 *       only (a slot at or beyond count keeps what the buffer held: hand in zeros).  ckpt may be NULL here: no checkpoint is kept, for
 *       a forward that nobody differentiates.
 *   dhts_micro_rollout_bwd_ckpt_samples   the sweep of dMicroForwardLayer.backward (dmicro_lane.py:271-298, with the virtual-leader slot
 *       of dMicroLane.vectorize_input :130-153; the parameter gradient that of road/lane/_micro_lane.py:131-214 over
 *       IDM.compute_acceleration, model/micro/_idm.py:30-49), as dhts_micro_rollout_bwd_ckpt.  g_samples enters at the sampled steps
 *       only, and only at live probe slots (the dense sweep adds a g_hist row at every step).
 *   dhts_micro_rollout_fwd_jvp_samples    forward mode of the plain MicroLane rollout (road/lane/_micro_lane.py:131-214 over
 *       IDM.compute_acceleration, model/micro/_idm.py:30-49; the blocks those of road/lane/dmicro_lane.py:87-127), as
 *       dhts_micro_rollout_fwd_jvp.  The first launch alone writes samples; t_samples: probe slots at or beyond count exactly 0.
 * DHTS_E_INVALID, nothing dereferenced and nothing launched: whatever the sibling rejects (but a NULL ckpt of the forward), every < 1,
 * n_probes outside 1 .. capacity with a non-NULL list, a NULL samples / g_samples / t_samples when T / every > 0.
 * Blocks, segments and dynamic LDS are the siblings': dhts_micro_ckpt_plan and dhts_micro_fwd_jvp_plan hold for the sampled forms too
 * (the probe list needs no LDS: each thread reads its slot's column once, before its step loop).
 */
int dhts_micro_rollout_fwd_ckpt_samples(const dhts_micro_desc *d, int T, int segment, const float *p, const float *v, const int32_t *count,
                                        const double *params, const double *head, float *p_out, float *v_out, void *ckpt,
                                        const int32_t *probes, int n_probes, int every, float *samples, dhts_error *err, void *stream);
int dhts_micro_rollout_bwd_ckpt_samples(const dhts_micro_desc *d, int T, int segment, const void *ckpt, const int32_t *count,
                                        const double *params, const double *head, const float *g_p, const float *g_v, const int32_t *probes,
                                        int n_probes, int every, const float *g_samples, float *g_p_out, float *g_v_out, double *g_head,
                                        double *g_params, dhts_error *err, void *stream);
int dhts_micro_rollout_fwd_jvp_samples(const dhts_micro_desc *d, int T, int n_dir, const float *p, const float *v, const int32_t *count,
                                       const double *params, const double *head, const float *t_p, const float *t_v, const double *t_head,
                                       const double *t_params, float *p_out, float *v_out, float *t_p_out, float *t_v_out,
                                       const int32_t *probes, int n_probes, int every, float *samples, float *t_samples, dhts_error *err,
                                       dhts_error *err_jvp, void *stream);

/*
 * A RECORDED LEADER on the two tape-free paths: the lane's head vehicle (slot count - 1) follows a prescribed vehicle that moves, as
 * every other vehicle follows the slot in front of it.  The three entry points are the _samples ones above with head / g_head / t_head
 * replaced by
 *   lead          [T][L][2] float32: (p, v) of the vehicle in front of lane l's head AS THE HEAD SEES IT IN step t -- what S[k + 1] is
 *                 to follower k.  No virtual leader and no head gap exist: the head forms
 *                     dp = fabs((double)lead_p - p) - half_len        dv = v - (double)lead_v
 *                 calls the same idm_step, and the same collision / clamp rules and live-gap test (gap >= 1e-5) apply to it.
 *   lead_length   [L] DOUBLE or NULL: half_len = (lead_length[l] + the head's own length) / 2; NULL = the head's own length for both,
 *                 the value the head's half_len has in the siblings.  Not differentiated.
 *   g_lead        [T][L][2] float32, written: row t = the cotangent of lead[t], i.e. the (C1p[n], C1v[n]) the sweep forms for the slot
 *                 in front of the head at step t.  Nothing is folded back into the head.  EVERY row is written; rows of a lane without
 *                 a vehicle are exactly 0.
 *   t_lead        [K][T][L][2] float32 or NULL (zero): the tangents of lead per direction.  The head's length tangent carries its own
 *                 share only: -(t_len / 2) where the gap is live; g_params[5] of the head likewise.
 * and samples / g_samples / t_samples may be NULL: nothing is observed (samples and t_samples of _fwd_jvp_lead: both or neither).  A
 * dense history is probes = NULL, every = 1.  Otherwise their siblings' arguments, arithmetic, fault records and bits:
 *   dhts_micro_rollout_fwd_ckpt_lead   MicroLane.forward (_micro_lane.py:131-214) with the head's leader given per step, as
 *       dhts_micro_rollout_fwd_ckpt_samples; DHTS_FAULT_COLLISION also where the head meets a leader behind it (gap < 0).
 *   dhts_micro_rollout_bwd_ckpt_lead   the sweep of dMicroForwardLayer.backward (dmicro_lane.py:271-298) with the leader slot of
 *       dMicroLane.vectorize_input (:130-153) returned per step instead of folded, as dhts_micro_rollout_bwd_ckpt_samples.
 *   dhts_micro_rollout_fwd_jvp_lead    forward mode of the same rollout, as dhts_micro_rollout_fwd_jvp_samples.
 * Exactly 0: g_p_out, g_v_out, g_params and t_p_out, t_v_out, t_samples at slots at or beyond count; g_lead rows of an empty lane.
 * DHTS_E_INVALID, nothing dereferenced and nothing launched: whatever the sibling rejects (but NULL sample arrays), a NULL lead with
 * T > 0, a NULL g_lead with T > 0, one of samples / t_samples NULL and the other not.
 * Blocks, segments and dynamic LDS are the siblings': dhts_micro_ckpt_plan and dhts_micro_fwd_jvp_plan hold for these forms too (the
 * leader's state travels in the slot V of the hand-over arrays that the virtual leader's tangents use in the siblings).
 */
int dhts_micro_rollout_fwd_ckpt_lead(const dhts_micro_desc *d, int T, int segment, const float *p, const float *v, const int32_t *count,
                                     const double *params, const float *lead, const double *lead_length, float *p_out, float *v_out,
                                     void *ckpt, const int32_t *probes, int n_probes, int every, float *samples, dhts_error *err,
                                     void *stream);
int dhts_micro_rollout_bwd_ckpt_lead(const dhts_micro_desc *d, int T, int segment, const void *ckpt, const int32_t *count,
                                     const double *params, const float *lead, const double *lead_length, const float *g_p, const float *g_v,
                                     const int32_t *probes, int n_probes, int every, const float *g_samples, float *g_p_out, float *g_v_out,
                                     float *g_lead, double *g_params, dhts_error *err, void *stream);
int dhts_micro_rollout_fwd_jvp_lead(const dhts_micro_desc *d, int T, int n_dir, const float *p, const float *v, const int32_t *count,
                                    const double *params, const float *lead, const double *lead_length, const float *t_p, const float *t_v,
                                    const float *t_lead, const double *t_params, float *p_out, float *v_out, float *t_p_out, float *t_v_out,
                                    const int32_t *probes, int n_probes, int every, float *samples, float *t_samples, dhts_error *err,
                                    dhts_error *err_jvp, void *stream);

/*
 * THE TRAJECTORY-FIT LOSS inside the checkpointed pair: sum((hist - observed)^2) and its gradient without hist and without g_hist.
 * The two entry points are dhts_micro_rollout_fwd_ckpt / _bwd_ckpt (head given) or _fwd_ckpt_lead / _bwd_ckpt_lead without probes (lead
 * given; EXACTLY ONE of head and lead, lead_length only with lead) with hist / g_hist, samples / g_samples replaced by
 *   target   [T][L][2][V] float32, hist's indexing: target[t][l][0 / 1][k] = the observed (p, v) of slot k AFTER step t.  A NaN entry is
 *            not observed: it adds exactly 0 to sse and no cotangent.  Slots at or beyond count are never read.
 *   sse      [L][2] DOUBLE, written: per lane the sum over observed entries of the squared position residual, and of the squared speed
 *            residual.  The residual is the float32 difference x - target (what hist - observed is), squared and summed in double: each
 *            thread sums its own vehicle in step order, the workgroup combines the per-thread sums pairwise in a fixed order through
 *            LDS.  No atomics: two runs give the same bits.  T = 0 and an empty lane: 0.
 *   g_sse    [L][2] DOUBLE or NULL (zero): the cotangent of sse.  The reverse sweep adds (float)(2 g_sse[l][c]) * r -- r the same float32
 *            residual, recomputed from the replayed state; 0 for a NaN entry -- to the cotangent of slot k at step t where
 *            dhts_micro_rollout_bwd_ckpt adds g_hist[t][l][c][k], with the same float32 add.
 * and otherwise their siblings' arguments, arithmetic, fault records and bits (p_out, v_out and, for equal per-step cotangents, every
 * gradient):
 *   dhts_micro_rollout_fwd_ckpt_target   the rollout of dMicroForwardLayer.forward (dmicro_lane.py:230-269 = MicroLane.forward
 *       _micro_lane.py:131-214 + dMicroLane._backward :87-127) and the loss of example/inverse/micro.py:36-118 on its trajectory.  ckpt
 *       may be NULL: no checkpoint is kept (a loss evaluation that nobody differentiates).  A block smaller than the lane
 *       (DHTS_FAULT_CAPACITY): sse of the lane is NaN.
 *   dhts_micro_rollout_bwd_ckpt_target   the sweep of dMicroForwardLayer.backward (dmicro_lane.py:271-298, with the virtual-leader slot
 *       of dMicroLane.vectorize_input :130-153 folded into the head, or returned per step as g_lead; the parameter gradient that of
 *       road/lane/_micro_lane.py:131-214 over IDM.compute_acceleration, model/micro/_idm.py:30-49).  g_head with head, g_lead [T][L][2]
 *       with lead; g_params optional.
 * target is read once per direction, coalesced along k; nothing of size T x V is written.
 * DHTS_E_INVALID, nothing dereferenced and nothing launched: a bad descriptor, T < 0, head and lead both given or (T > 0) neither,
 * lead_length / g_lead with head, g_head with lead, a NULL target or ckpt (reverse) or g_lead (with lead) when T > 0, a NULL p / v /
 * params / p_out / v_out / sse / g_p / g_v / g_p_out / g_v_out, a segment outside 0 .. the max_segment of dhts_micro_ckpt_target_plan.
 * dhts_micro_ckpt_target_plan: dhts_micro_ckpt_plan's eight entries for these two kernels.  The reverse kernel's ring holds two more
 * floats per vehicle-step (the finished cotangent pair), so max_segment and the default segment (the same rule: the longest that keeps
 * 16 wavefronts resident on a CU by LDS, at most 16) are shorter; segment 0 at the two entry points is THIS plan's default.  The
 * checkpoint buffer is dhts_micro_ckpt_bytes of the resolved segment plan[1].
 */
int dhts_micro_ckpt_target_plan(const dhts_micro_desc *d, int T, int want_params, int segment, int32_t plan[8]);
int dhts_micro_rollout_fwd_ckpt_target(const dhts_micro_desc *d, int T, int segment, const float *p, const float *v, const int32_t *count,
                                       const double *params, const double *head, const float *lead, const double *lead_length,
                                       float *p_out, float *v_out, void *ckpt, const float *target, double *sse, dhts_error *err,
                                       void *stream);
int dhts_micro_rollout_bwd_ckpt_target(const dhts_micro_desc *d, int T, int segment, const void *ckpt, const int32_t *count,
                                       const double *params, const double *head, const float *lead, const double *lead_length,
                                       const float *g_p, const float *g_v, const float *target, const double *g_sse, float *g_p_out,
                                       float *g_v_out, double *g_head, float *g_lead, double *g_params, dhts_error *err, void *stream);

/*
 * A RING ROAD on the two tape-free paths: the lane is closed.  Its n = clamp(count[l], 0, V) vehicles drive on a ring of circumference
 * ring[l], and the head (slot n - 1) follows the IMAGE OF THE TAIL (slot 0) one circumference ahead, as every other vehicle follows the
 * slot in front of it.  The five entry points are the _lead ones and the _target pair above, each with the same argument order, with
 * (lead, lead_length) -- and head, in the target pair -- replaced by
 *   ring          [L] DOUBLE, the circumference of each lane's ring in metres; read once per lane; NOT differentiated.  Positions stay
 *                 UNWRAPPED: no modulo is taken anywhere, p keeps growing as on an open lane, and the caller wraps for display.
 * and without g_head / g_lead / t_head / t_lead: none of them exists.  In step t the head sees
 *       image = ((float)((double)p_tail + ring[l]), v_tail)        (p_tail, v_tail): the tail's float32 state BEFORE step t
 * which is exactly what S[k + 1] is to follower k, and forms with the expressions of every follower
 *       dp = fabs((double)image_p - p) - half_len        dv = v - (double)image_v        half_len = (length[slot 0] + length[head]) / 2
 * calls the same idm_step, and the same collision / clamp rules and live-gap test (gap >= 1e-5) apply to it.  The tail's length is a
 * LIVE parameter here (lead_length is not).  n = 1: the vehicle follows its own image, half_len is its own length.  n = 0: nothing
 * happens, the state passes through and every gradient and tangent of the lane is exactly 0.
 *   reverse mode   the cotangent (C1p[n], C1v[n]) the sweep forms for the slot in front of the head is added to the TAIL's cotangent in
 *                  the same sweep step (the float cast has derivative 1, like every float32 state store).  Nothing returns to the head
 *                  (no virtual leader) and no per-step row is written.  With g_params the head's gap term is live, as with lead, and the
 *                  tail's length also collects the head's share: g_params[5][slot 0] = -0.5 (A[0] + A[n - 1]), A[k] the gap sum of
 *                  slot k; n = 1: -A[0].
 *   forward mode   the tangents of the image are the tail's state tangents before the step; the head's length tangent is
 *                  -(t_len[head] + t_len[tail]) / 2 where the gap is live.
 * A ring too short for its vehicles is the caller's error: it shows as the sticky DHTS_FAULT_COLLISION record of the siblings, same
 * step, lane and vehicle rules.  samples / g_samples / t_samples may be NULL: nothing is observed (samples and t_samples of
 * _fwd_jvp_ring: both or neither).  Otherwise the siblings' arguments, arithmetic, fault records and bits:
 *   dhts_micro_rollout_fwd_ckpt_ring          MicroLane.forward (_micro_lane.py:131-214) with the head's leader taken from the tail.
 *   dhts_micro_rollout_bwd_ckpt_ring          the sweep of dMicroForwardLayer.backward (dmicro_lane.py:230-298) with the leader slot of
 *       dMicroLane.vectorize_input (:130-153) returned to the tail instead of folded into the head.
 *   dhts_micro_rollout_fwd_jvp_ring           forward mode of the same rollout, as dhts_micro_rollout_fwd_jvp_lead.
 *   dhts_micro_rollout_fwd_ckpt_target_ring / _bwd_ckpt_target_ring   the trajectory fit above on the ring (dhts_micro_ckpt_target_plan).
 * DHTS_E_INVALID, nothing dereferenced and nothing launched: whatever the sibling rejects (but NULL sample arrays), a NULL ring.
 * Blocks, segments and dynamic LDS are the siblings': dhts_micro_ckpt_plan, dhts_micro_ckpt_target_plan and dhts_micro_fwd_jvp_plan hold
 * as they are (the image travels in slot V of the hand-over arrays, written by the tail's thread; one LDS-only barrier per step).
 * Not built: the taped kernels and the taped JVP, a gradient or tangent of ring, wrap-around of positions, the network kernels.
 */
int dhts_micro_rollout_fwd_ckpt_ring(const dhts_micro_desc *d, int T, int segment, const float *p, const float *v, const int32_t *count,
                                     const double *params, const double *ring, float *p_out, float *v_out, void *ckpt,
                                     const int32_t *probes, int n_probes, int every, float *samples, dhts_error *err, void *stream);
int dhts_micro_rollout_bwd_ckpt_ring(const dhts_micro_desc *d, int T, int segment, const void *ckpt, const int32_t *count,
                                     const double *params, const double *ring, const float *g_p, const float *g_v, const int32_t *probes,
                                     int n_probes, int every, const float *g_samples, float *g_p_out, float *g_v_out, double *g_params,
                                     dhts_error *err, void *stream);
int dhts_micro_rollout_fwd_jvp_ring(const dhts_micro_desc *d, int T, int n_dir, const float *p, const float *v, const int32_t *count,
                                    const double *params, const double *ring, const float *t_p, const float *t_v, const double *t_params,
                                    float *p_out, float *v_out, float *t_p_out, float *t_v_out, const int32_t *probes, int n_probes,
                                    int every, float *samples, float *t_samples, dhts_error *err, dhts_error *err_jvp, void *stream);
int dhts_micro_rollout_fwd_ckpt_target_ring(const dhts_micro_desc *d, int T, int segment, const float *p, const float *v,
                                            const int32_t *count, const double *params, const double *ring, float *p_out, float *v_out,
                                            void *ckpt, const float *target, double *sse, dhts_error *err, void *stream);
int dhts_micro_rollout_bwd_ckpt_target_ring(const dhts_micro_desc *d, int T, int segment, const void *ckpt, const int32_t *count,
                                            const double *params, const double *ring, const float *g_p, const float *g_v,
                                            const float *target, const double *g_sse, float *g_p_out, float *g_v_out, double *g_params,
                                            dhts_error *err, void *stream);

/*
 * The GAUSS-NEWTON NORMAL EQUATIONS of a trajectory fit inside the fused forward + tangent kernel: forward mode's counterpart of the
 * _ckpt_target pair.  dhts_micro_rollout_fwd_jvp_gn runs the rollout and its n_dir tangent directions as dhts_micro_rollout_fwd_jvp_samples
 * / _lead / _ring do -- the same arguments, arithmetic, fault records and bits of (p_out, v_out, t_p_out, t_v_out) -- and, instead of
 * writing samples / t_samples, sums over them against
 *   target   [T / every][L][2][n] float32, the layout of samples (n = n_probes, or V with probes NULL; probes NULL and every 1 is
 *            hist's indexing [T][L][2][V]): the observed (p, v) of probe slot i after step (j + 1) every - 1.  A NaN entry is NOT
 *            OBSERVED and adds exactly 0 to all three sums; a column whose slot is at or beyond count[l] is never read.
 * With x the float32 sample, r = x - target in float32, and t_a the float32 tangent of x in direction a (what t_samples would hold):
 *   sse      [L][2] double      sse[l][c] = sum of (double)r (double)r over the observed entries of plane c: dhts_micro_rollout_fwd_ckpt_target's
 *                               definition and, with probes NULL and every 1, its bits
 *   jtr      [L][n_dir] double          jtr[l][a]    = sum over the observed entries of lane l, BOTH planes, of (double)t_a (double)r
 *   jtj      [L][n_dir][n_dir] double   jtj[l][a][b] = the same sum of (double)t_a (double)t_b; both triangles are written, bit-symmetric
 * Every product is exact in double.  A thread sums its own vehicle's terms in step order (p's, then v's), the workgroup combines the
 * slots by the target forms' fixed-order pairwise tree: no atomics, two runs give the same bits.  T / every = 0 and an empty lane give
 * zeros.  No weights but the NaN mask; no gradient of the sums (reverse mode has the _ckpt_target pair).
 *   head, or lead (lead_length), or ring    exactly one is non-NULL and names the form (T = 0: all three may be NULL); t_head only with
 *            head, t_lead only with lead, each [n_dir][...] as in the sibling, NULL: zero.
 * Launches: a launch carries up to plan[1] directions.  n_dir <= plan[1]: one launch.  Otherwise the directions are cut into blocks of
 * plan[1] / 2 and every PAIR of blocks gets a launch (a cross product needs both directions in one launch): with plan[1] = 4, n_dir 5, 6:
 * 3 launches, 7, 8: 6.  Each recomputes the primal and writes its directions' rows of jtr and pairs of jtj in place; an entry written by
 * several launches receives the same bits from each.  The first alone writes p_out, v_out, sse and is handed err.
 * dhts_micro_fwd_jvp_gn_plan: plan[0] block size (the lane rounded up to 64: one vehicle per thread)
 *                             plan[1] direction slots of the widest kernel held for this lane and want_params: the widest whose
 *                                     compiler listing has no scratch and no register spill (the accumulators are 2 + K + K (K + 1) / 2
 *                                     doubles per thread): 4, but 2 with want_params for a lane of more than 512 slots
 *                             plan[2] launches for n_dir, 0: plan[1] cannot carry n_dir (plan[1] = 1 carries n_dir = 1 only)
 *                             plan[3] dynamic LDS bytes of the widest launch (the siblings': the sums are combined in the same bytes)
 *                             plan[4] directions per block of the pair scheme (n_dir where one launch takes them all)
 *                             plan[5] the block bound the widest launch's kernel is compiled for (512 or 1024)
 * DHTS_E_INVALID, nothing dereferenced and nothing launched: whatever the siblings reject; more or fewer than one of head, lead, ring
 * (T > 0); t_head without head, t_lead or lead_length beside head or ring, or without lead where T > 0; a NULL target with T / every > 0; a NULL sse, jtr or jtj; an n_dir
 * with plan[2] = 0.  A block smaller than the lane: DHTS_FAULT_CAPACITY, the lane's sse, jtr and jtj NaN.
 */
int dhts_micro_rollout_fwd_jvp_gn(const dhts_micro_desc *d, int T, int n_dir, const float *p, const float *v, const int32_t *count,
                                  const double *params, const double *head, const float *lead, const double *lead_length,
                                  const double *ring, const float *t_p, const float *t_v, const double *t_head, const float *t_lead,
                                  const double *t_params, float *p_out, float *v_out, float *t_p_out, float *t_v_out,
                                  const int32_t *probes, int n_probes, int every, const float *target, double *sse, double *jtr,
                                  double *jtj, dhts_error *err, dhts_error *err_jvp, void *stream);
int dhts_micro_fwd_jvp_gn_plan(const dhts_micro_desc *d, int T, int n_dir, int want_params, int32_t plan[8]);

int dhts_micro_step_fwd(const dhts_micro_desc *d,
                        const float *p, const float *v, const int32_t *count, const double *params, const double *head,
                        float *p_out, float *v_out, float *tape, dhts_error *err, void *stream);
/* The same step in the float32 TENSOR ladder: what the reference's plain MicroLane (road/lane/_micro_lane.py:131-214 over
 * model/micro/_idm.py:6-50) computes when its vehicle states are torch tensors -- every operation rounds to float32, Python float
 * operands are cast first, pow(x, 2.0) = x * x, pow(x, 4.0) = powf.  itscp `micro` mode steps its lanes that way in differentiable
 * episodes (example/control/itscp/_env.py:484-498).  Same arguments, same tape (the analytic Jacobian blocks at the same operands:
 * what autograd differentiates), same reverse operator dhts_micro_step_bwd. */
int dhts_micro_step_fwd_tensor(const dhts_micro_desc *d,
                               const float *p, const float *v, const int32_t *count, const double *params, const double *head,
                               float *p_out, float *v_out, float *tape, dhts_error *err, void *stream);
/* The same step when only the lane's HEAD GAP is a float32 tensor: dMicroLane.detach_vehicle (road/lane/dmicro_lane.py:228-250) turns the
 * vehicles' states into Python floats but leaves head_position_delta / head_speed_delta alone, so with a tensor gap (a differentiable
 * itscp hybrid episode: the signal blend of example/control/itscp/_simulator.py:260-263; a plain network: a leader in sight) the head
 * vehicle's IDM.compute_acceleration and Euler step run in mixed arithmetic -- double where two Python floats meet, float32 where the
 * tensor is involved -- and the followers' in double as in dhts_micro_step_fwd.  head [L][2] double holds the tensor's float32 values.
 * Same arguments, same tape, same reverse operator. */
int dhts_micro_step_fwd_tensor_head(const dhts_micro_desc *d,
                                    const float *p, const float *v, const int32_t *count, const double *params, const double *head,
                                    float *p_out, float *v_out, float *tape, dhts_error *err, void *stream);
/* The single-step reverse keeps the operator form of dMicroForwardLayer.backward: the cotangent of the virtual
 * leader slot is NOT folded back into the head vehicle; g_head [L][2] DOUBLE returns it raw as (g_p[V], g_s[V]). */
int dhts_micro_step_bwd(const dhts_micro_desc *d, const float *tape, const int32_t *count,
                        const float *g_p, const float *g_v,
                        float *g_p_out, float *g_v_out, double *g_head, dhts_error *err, void *stream);


/* ---- macro road network with differentiable signals (itscp `macro` mode) -------------------------------------------
 * One fused rollout of R independent replicas of a signalised network of ARZ lanes: replaces, per replica, what
 * ItscpEnv._simulate does with ItscpRoadNetwork.forward (example/control/itscp/_env.py:620-768, 885-962;
 * _simulator.py:56-137; road/network/road_network.py:79-111, 299-387) and ItscpEnv._reward (_env.py:770-797):
 * per step  signals from the action -> ghost cells of every lane from its neighbours' time-n edge cells, blended between
 * green and red values -> one ARZ step per lane -> queue-length loss (running-mean-scaled sigmoid, _env.py:586-618).
 * Lanes start empty.  Tables (device pointers) are built on the host (dhts/network.py):
 *   lane_ncell, lane_off, sig_kind (0 always green, 1 west-east phase, 2 north-south phase), inter [L] int32; lane_dx [L]
 *   DOUBLE; left_src / left_gate / right_src [T][L] int32 and schedule [T][L] DOUBLE, per replica when replica_stride
 *   (elements between replicas) is non-zero, else shared.  The loss' RunningMean(100 000) window slides once T * n_cells exceeds it
 *   (the samples that leave are re-read from the state history).  Limits: n_cells + n_lanes <= 1024 (one workgroup per replica), n_action <= 1024, at most 4 upstream / 4 downstream lanes per lane.
 */
typedef struct dhts_net_desc {
    int32_t n_replicas, n_lanes, n_cells, n_steps, n_inter_sq, frames_per_phase, n_action;
    double dt, u_max, static_speed, vehicle_length;
} dhts_net_desc;
typedef struct dhts_net_tables {
    const int32_t *lane_ncell, *lane_off, *sig_kind, *inter;
    const double *lane_dx;
    const int32_t *left_src, *left_gate, *right_src;
    const double *schedule;
    int64_t replica_stride;
    /* static adjacency in CSR form, neighbour ids ascending: next lanes of lane l = nxt_idx[nxt_ptr[l] .. nxt_ptr[l+1]),
     * previous lanes likewise (used by the reverse sweep to route ghost cotangents without searching) */
    const int32_t *nxt_ptr, *nxt_idx, *prv_ptr, *prv_idx;
    int32_t n_edges;
} dhts_net_tables;
size_t dhts_net_macro_hist_bytes(const dhts_net_desc *d);   /* state history [R][T+1][4][C] float32 */
size_t dhts_net_macro_tape_bytes(const dhts_net_desc *d);   /* Jacobian tape [R][T][3][Cp][4] float32 */
/* What the fused pair below launches for this network (the evaluation kernel takes the reverse sweep's block, bound 1024):
 * plan[0] forward block size     plan[1] 1 = the forward runs the loss on wavefronts of its own (pad64(max(C + L, n_action)) + pad64(C)
 * threads fit 1024), 0 = behind the physics role     plan[2] forward launch bound (512, 640 or 1024 threads)
 * plan[3] reverse block size = pad64(max(C + L, n_action))     plan[4] reverse launch bound (512 or 1024)     plan[5..7] 0 */
int dhts_net_macro_plan(const dhts_net_desc *d, int32_t plan[8]);
/* action [R][n_action]; out: hist, tape, kc [R][T][C] (loss sigmoid constants), queue [R][T][L] (loss terms q^2 dt),
 * reward [R] float32 = - sum of the queue terms; workspace [R][T][2 L] float32 (kept for the reverse sweep) */
int dhts_net_macro_rollout_fwd(const dhts_net_desc *d, const dhts_net_tables *t, const float *action, float *hist, float *tape,
                               float *kc, float *queue, float *reward, float *workspace, dhts_error *err, void *stream);
/* An EVALUATION episode of the same R replicas: ItscpEnv.step(action, False), what Trainer.evaluate runs every num_eval_epoch
 * epochs (example/control/trainer.py:73-75, 94-142).  The lanes step exactly as above; the thresholds are hard: signals
 * float(a > progress) / float(progress > a) (_env.py:928-960), downstream ghost float(signal > 0.5) (_simulator.py:128-137),
 * is_static = 1.0 if speed < static_speed else 0.0 without a running mean (_env.py:607-617).  Nothing is kept for a reverse
 * sweep.  out: queue [R][T][L], reward [R]. */
int dhts_net_macro_rollout_eval(const dhts_net_desc *d, const dhts_net_tables *t, const float *action, float *queue, float *reward,
                                dhts_error *err, void *stream);
/* hist, tape, kc, queue, workspace from the forward; g_reward [R] (NULL = ones) -> g_action [R][n_action] */
int dhts_net_macro_rollout_bwd(const dhts_net_desc *d, const dhts_net_tables *t, const float *action, const float *hist,
                               const float *tape, const float *kc, const float *queue, const float *g_reward, float *g_action,
                               const float *workspace, dhts_error *err, void *stream);

/* ---- Macro road networks of ANY size, step by step (round 4) ---------------------------------------------------------------
 * The rollouts above keep a replica in one workgroup (cells + lanes <= 1024); the reference builds grids of any size
 * (example/control/itscp/_env.py:221-439).  A larger network steps as RoadNetwork.forward does (road_network.py:57-111), one
 * operator call per step for ALL lanes: dhts_net_ghosts_fwd turns the state before step `step` into every lane's two ghost
 * cells -- the connected neighbour's edge cell, the inflow schedule of a source lane or the stored downstream ghost of a sink
 * lane, blended between green and red by the signals of that step (ItscpRoadNetwork.setup_macro_boundary,
 * _simulator.py:42-60; signals _env.py:885-962) -- in the layout dhts_macro_step_fwd takes its ghosts in, the lanes then step
 * as batches of that operator (lanes of equal cells and cell length), and dhts_net_ghosts_bwd routes the operator's ghost
 * cotangents (dhts_macro_step_bwd's g_ghost) back: to the neighbours' edge cells (r, y), to the stored ghosts and to the action.
 * d / t as for dhts_net_macro_rollout_fwd with n_replicas = 1 (lane_off / lane_ncell give the edge cells; rows `step` of
 * left_src / left_gate / right_src / schedule are read).  r, y, u [C] = the state before the step (u = u(r, y) as the operator
 * left it); own_in / own_out [L][2] = the lanes' stored downstream ghosts (r, u) before / after (initially (0, u_max));
 * ghost [L][2][4] = (left, right) x (r, y, u, u_eq), a source lane's left quad in the double encoding dhts_macro_step_fwd documents;
 * hard != 0 = an evaluation episode's thresholds.
 * _bwd: g_ghost [L][2][2] double (d / d ghost (r, y)), g_own_in [L][2] = cotangent of own_out; g_own_out [L][2] is written;
 * g_r, g_y [C] and g_action [n_action] are ACCUMULATED into (edge cells in a fixed order: bit-repeatable); inter_ptr [sq + 1],
 * inter_idx = the ghost slots (2 lane + side) of every intersection in ascending order; scratch [L][2][4] float32. */
int dhts_net_ghosts_fwd(const dhts_net_desc *d, const dhts_net_tables *t, int step, int hard, const float *action, const float *r,
                        const float *u, const float *own_in, float *own_out, float *ghost, void *stream);
int dhts_net_ghosts_bwd(const dhts_net_desc *d, const dhts_net_tables *t, const int32_t *inter_ptr, const int32_t *inter_idx, int step,
                        const float *action, const float *r, const float *y, const float *u, const float *own_in,
                        const double *g_ghost, const float *g_own_in, float *g_own_out, float *g_r, float *g_y, float *g_action,
                        float *scratch, void *stream);

/* ---- HYBRID road network (itscp `hybrid` mode): macro lanes, micro lanes and the hand-offs between them -----------------
 * As the macro network rollout, with lanes that are either ARZ cell lanes or IDM vehicle lanes and, after every step,
 * the conversions of road/network/conversion.py:11-215 in lane-id order (RoadNetwork.conversion, road_network.py:113-170):
 *   macro -> micro  flux capacitor of the last cell (+= r u dt), spawn of a default vehicle (p = 0, v = u_last, ancillary
 *                   a = capacitor) once it holds one vehicle length and the successor has that much free space (:16-73)
 *   micro -> macro  the head vehicle past the lane end by more than its length is deposited into the successor's first
 *                   cells (density a/len * overlap/dx, straight-through clamp, cell speed = vehicle speed) (:76-171)
 *   micro -> micro  lane change at p >= L (:175-200);  micro -> none at p >= L (:203-215)
 * plus the head gap of every occupied micro lane: leader further along the route (road_network.py:429-580) blended with the
 * red-light stop line by position-weighted neighbour signals (_simulator.py:139-276), and the vehicles' terms of the queue
 * loss (_env.py:694-725).  Vehicles use MicroVehicle.default_micro_vehicle (micro_vehicle.py:31-72).
 * One workgroup per replica; the (few) scalar operations of the micro side run on an extra wavefront (one lane per micro
 * lane; the hand-off events serially) and are recorded, with their partial derivatives, on a per-replica record stream that
 * the reverse sweep replays backwards.
 * Extra tables (device pointers):
 *   lane_macro [L] int32 (1 = cells, 0 = vehicles; micro lanes have 0 cells), lane_len [L] DOUBLE,
 *   left_src -3 = own stored upstream ghost (single upstream lane is micro), right_src -1 also when the single downstream
 *   lane is micro, conv_next [T][L] int32 = the step's macro-route successor of a macro lane (per replica like left_src),
 *   routes [n_routes][route_stride] int32 (-1 padded), grouped by their first lane, and route_ptr [L + 1] int32 (rows
 *   route_ptr[m] .. route_ptr[m+1] start on micro lane m): the k-th vehicle spawned onto lane m takes row
 *   route_ptr[m] + k mod (rows of m).  The reference draws a route with np.random at spawn time (road_network.py:604-646);
 *   callers pre-draw them (dhts/network.py: group_routes keeps a recorded spawn order intact).
 * Limits: n_cells + n_lanes <= 960 (n_cells = 0 is allowed: an all-micro network), <= 64 micro lanes, <= 16 spawning lanes, <= lane_capacity vehicles per micro lane (16 unless asked for: below), <= 48 tape
 * records per micro lane and step (2 lane_capacity + 32 with a larger lane_capacity) -- fewer when more than ~20 micro lanes share the workgroup's LDS staging, e.g. 18 at 64
 * micro lanes beside 288 cells; a lane with k vehicles stages ~8 + 2 k (DHTS_FAULT_CAPACITY beyond), <= 128 vehicles per replica and episode, route_stride <= 32; records_per_step (average budget of the record stream,
 * 0 = 512).  loss_steps: only the first loss_steps steps enter reward_cut and the gradient (<= 0: all).
 */
typedef struct dhts_hybrid_tables {
    dhts_net_tables net;
    const int32_t *lane_macro;
    const double *lane_len;
    const int32_t *conv_next;
    const int32_t *routes;
    const int32_t *route_ptr;
    int32_t n_routes, route_stride, records_per_step, loss_steps;
    int32_t n_micro;            /* number of micro lanes (zeros of lane_macro); sizes the kernels' LDS staging */
    /* micro SOURCE lanes -- micro lanes without an upstream lane; itscp `micro` mode, where every lane is an IDM lane and
     * n_cells = 0 (ItscpRoadNetwork.setup_micro_boundary, _simulator.py:153-174): at the boundary of a step such a lane admits
     * a waiting vehicle (position 0, speed 0) when it has more than half a vehicle length of room at its entrance and the
     * host's draw np.random.random() is below the step's inflow schedule[t][lane].  The draws are data: `draws` is the stream
     * in call order (one draw per source lane with room, lanes in id order, steps in order), n_draws its length (a run that
     * needs more raises DHTS_FAULT_CAPACITY), draws_stride the elements between replicas (0 = shared).  The k-th vehicle admitted
     * to lane m takes route row route_ptr[m] + k (no wrap-around: the rows are the lane's waiting list in admission order, and an
     * exhausted list admits nobody).  lane_source [L] int32 (1 = source lane) or NULL = the network has none.
     * (Which arithmetic the IDM lanes step in is micro_tensor_ladder's business, below -- not inferred from lane_source.) */
    const int32_t *lane_source;
    const double *draws;
    int32_t n_draws;
    int64_t draws_stride;
    /* vehicles a micro lane holds at once: 0 (= 16), 16, 32, 64 or 128.  A per-launch LDS sizing like n_micro (4 bytes per slot and
     * micro lane, plus staging for one IDM record and one loss seed per vehicle and step, as far as the 160 KB go): the reference's
     * lanes are unbounded (_micro_lane.py:53-113), an episode that needs more than the launch was sized for ends in
     * DHTS_FAULT_CAPACITY and the caller retries with a larger value (ItscpEnv.step does) or runs lane by lane. */
    int32_t lane_capacity;
    /* 1 = the network's IDM lanes are the reference's PLAIN autodiff MicroLane objects on torch tensors -- itscp `micro` mode
     * (example/control/itscp/_env.py:484-498; road/lane/_micro_lane.py:131-214 evaluated by torch): in differentiable episodes the IDM
     * step follows that float32 TENSOR ladder operation by operation (csrc/idm_device.hpp idm_step_f32).  0 = dMicroLane lanes (every
     * other network, with or without source lanes): the analytic operator's float64 ladder (dmicro_lane.py:87-127), the head vehicle in
     * mixed arithmetic while its gap is a tensor.  The host says which (ItscpEnv's `micro` branch sets 1). */
    int32_t micro_tensor_ladder;
    /* The vehicles' IDM attributes, [n_routes][6] DOUBLE (device) beside the route table -- row i belongs to the vehicle that takes
     * route row i: (accel_max, accel_pref, target_speed, min_space, time_pref, length) as MicroVehicle holds them
     * (road/vehicle/micro_vehicle.py:5-28; random_micro_vehicle :75-121) -- or NULL: every vehicle is a
     * MicroVehicle.default_micro_vehicle(speed_limit) (:31-72), which is all the reference's network code ever builds
     * (road/network/conversion.py:51, road_network.py:582-591).  Rows are reused with their routes (the k-th vehicle spawned onto
     * lane m takes row route_ptr[m] + k mod rows of m).  length must equal the descriptor's vehicle_length (the hand-offs and the
     * loss use one length; both of the reference's factories give DEFAULT_VEHICLE_LENGTH). */
    const double *veh_params;
    /* Replicas per compute unit of the fused kernels for THIS set of tables: 0 = as DHTS_OPT_HYB_PACK says (default: two when the batch
     * has more replicas than the device has units), 1 = two whenever the plan fits, -1 = one.  A caller that met DHTS_FAULT_CAPACITY under
     * the packed plan (its record staging area holds about a third of the unpacked plan's records per lane and step: dhts_net_hybrid_plan plan[2]) retries with -1 (dhts.ops does). */
    int32_t two_per_cu;
} dhts_hybrid_tables;
size_t dhts_net_hybrid_workspace_bytes(const dhts_net_desc *d, const dhts_hybrid_tables *t);
/* What dhts_net_hybrid_rollout_fwd / _bwd would launch for (d, t) under the current DHTS_OPT_HYB_PACK (no device work): plan[0] = 1
 * when two replicas share a compute unit, [1] threads per workgroup, [2] records a micro lane can stage per step, [3] / [4]
 * bytes of LDS of the forward / reverse kernel, [5] lanes with a range of temporaries, [6] records a step may hold, [7] compute
 * units of the current device.  (No reference counterpart: the reference steps one environment in one Python thread,
 * example/control/trainer.py:168-204.) */
int dhts_net_hybrid_plan(const dhts_net_desc *d, const dhts_hybrid_tables *t, int32_t plan[8]);
/* bytes of the hybrid kernels' Jacobian tape: float32 [R][T][NIp][2][4], NIp = n_cells + n_lanes rounded up to 64: per interface
 * slot (a lane's n + 1 interfaces, lanes in id order, micro lanes own none) the two 2x2 products A = flux'(Q_0) dQ_0/dQ_L and
 * B = flux'(Q_0) dQ_0/dQ_R of dMacroLane._backward (dmacro_lane.py:116-124); the reverse sweep forms the cell blocks
 * dqs[a][0..2] (:126-129) from them.  (The macro-network kernels keep the blocks themselves: dhts_net_macro_tape_bytes.) */
size_t dhts_net_hybrid_tape_bytes(const dhts_net_desc *d);
/* hist / kc / queue / reward as in the macro rollout (kc rows of micro lanes do not exist: they have no cells); tape:
 * dhts_net_hybrid_tape_bytes;
 * counts [R][4] int32 = (vehicles spawned, vehicles deposited, records written, 0) */
int dhts_net_hybrid_rollout_fwd(const dhts_net_desc *d, const dhts_hybrid_tables *t, const float *action, float *hist,
                                float *tape, float *kc, float *queue, float *reward, int32_t *counts, void *workspace,
                                dhts_error *err, void *stream);
/* An EVALUATION episode (see dhts_net_macro_rollout_eval) of the hybrid network: additionally a head vehicle takes the green
 * head gap when the signal of its own lane is >= 0.5 and the red-light gap otherwise (_simulator.py:208-232, 264-276: scores
 * 0 / 1 / 0, no running mean), and a vehicle is static when its speed is below static_speed (_env.py:709-717).  Steps, hand-offs
 * and capacities as in dhts_net_hybrid_rollout_fwd; no records, tape, history or workspace.  out: queue [R][T][L], reward [R],
 * counts [R][4] = (vehicles spawned, vehicles deposited, 0, 0). */
int dhts_net_hybrid_rollout_eval(const dhts_net_desc *d, const dhts_hybrid_tables *t, const float *action, float *queue,
                                 float *reward, int32_t *counts, dhts_error *err, void *stream);
int dhts_net_hybrid_rollout_bwd(const dhts_net_desc *d, const dhts_hybrid_tables *t, const float *action, const float *hist,
                                const float *tape, const float *kc, const float *queue, const float *g_reward,
                                float *g_action, const void *workspace, dhts_error *err, void *stream);

/* ---- the same kernels for a PLAIN road network with given initial state: example/inverse/hybrid.py ----------------------------
 * RoadNetwork.forward of the reference without the itscp layer (road/network/road_network.py:79-111, 299-362, 429-580): no
 * signals and no inflow schedules -- a ghost is the connected macro lane's edge cell or the lane's own STORED ghost, unblended
 * (get_macro_boundary), a head vehicle's gap is the one to its leader along its route (setup_micro_boundary) -- lanes that start
 * from a GIVEN state, and taps on the FINAL state instead of the queue loss: what example/inverse/hybrid.py:37-146 and
 * _inverse.py:91-99, 185-242 run T x (3 operator calls + host conversions) for.
 *   plain       1 = the plain network above (tables: sig_kind all 0, left_src / right_src = neighbour lane or -3 / -1 for the
 *               stored ghost, schedule unused); 0 = the itscp semantics of dhts_net_hybrid_rollout_fwd with the extra inputs
 *   state0      [R][4][C] float32 (r, y, u, u_eq) of every cell at step 0 (NULL = empty road: r = y = 0, u = u_eq = u_max)
 *   ghost0      [R][L][4] float32 (r, u) of each lane's stored upstream ghost, (r, u) of its stored downstream ghost
 *               (NULL = (0, u_max) both: set_leftmost_cell / set_rightmost_cell defaults)
 *   veh_out     [R][128][4] float32 out: (lane id or -1 once it left the network, position, speed, ancillary a) of every
 *               vehicle in spawn order (rows beyond counts[0] are not written)
 *   events      [R][256][2] int32 out: (step, kind) of the hand-off events in order, kind 0 = macro -> micro spawn, 1 = micro ->
 *               macro deposit; counts[3] = their number (NULL = not kept)
 * Reverse: g_stateT [R][3][C] cotangent of the final (r, y, u) per cell and g_veh [R][128][2] cotangent of the final (position,
 * speed) of vehicle k (either may be NULL) enter beside g_reward (NULL = ones, as above; pass zeros for a pure state tap);
 * g_state0 [R][3][C] out = cotangent of the initial (r, y, u) -- u collects what reads the GIVEN speed at step 0 (ghosts of
 * neighbouring lanes, a flux capacitor); the initial y = r (u - u_eq(r)) is the caller's (dhts_macro_state_from_ru_bwd). */
typedef struct dhts_hybrid_state_io {
    int32_t plain;
    const float *state0;
    const float *ghost0;
    float *veh_out;
    int32_t *events;
} dhts_hybrid_state_io;
int dhts_net_hybrid_state_rollout_fwd(const dhts_net_desc *d, const dhts_hybrid_tables *t, const dhts_hybrid_state_io *io,
                                      const float *action, float *hist, float *tape, float *kc, float *queue, float *reward,
                                      int32_t *counts, void *workspace, dhts_error *err, void *stream);
int dhts_net_hybrid_state_rollout_bwd(const dhts_net_desc *d, const dhts_hybrid_tables *t, int32_t plain, const float *action,
                                      const float *hist, const float *tape, const float *kc, const float *queue,
                                      const float *g_reward, const float *g_stateT, const float *g_veh, float *g_action,
                                      float *g_state0, const void *workspace, dhts_error *err, void *stream);

/* ---- Road networks of ANY size and ANY mix of ARZ / IDM lanes, step by step (round 5) ------------------------------------------
 * dhts_net_hybrid_rollout_* keep a replica in one workgroup (cells + lanes <= 960, <= 64 IDM lanes, <= 128 vehicles); the
 * reference's environment builds any grid in any mode (example/control/itscp/_env.py:221-506: `--lane_length`, `--n_lane`,
 * `--n_intersection` are free).  dhts_netstep_rollout_fwd / _bwd run such an episode step by step, every step a handful of
 * launches over flat device arrays, all T steps inside ONE call (no host round trip, no per-step Python):
 *   boundary   ghost cells of every ARZ lane (ItscpRoadNetwork.setup_macro_boundary, _simulator.py:56-137) | admission of
 *              waiting vehicles on micro source lanes (:153-174), head gap of every occupied IDM lane (:139-276 over
 *              RoadNetwork.setup_micro_boundary, road_network.py:429-580; forward-mode duals w.r.t. the head vehicle, its
 *              leader and the three signals it can see) and the IDM step of every vehicle (dMicroForwardLayer,
 *              dmicro_lane.py:230-269) -- one launch;
 *   lanes      dhts_macro_step_fwd once per group of ARZ lanes of equal (cells, cell length): dMacroForwardLayer for the batch;
 *   hand-offs  flux capacitors, then spawn / lane change / despawn / deposit in lane-id order (RoadNetwork.conversion,
 *              road_network.py:113-170; conversion.py:11-215) with an event list for the reverse sweep, then the queue loss of
 *              the committed state with its RunningMean(100 000) (_env.py:586-618, 664-742) -- one launch.
 * The reverse sweep undoes them newest first (loss taps -> events -> IDM / head gaps -> dhts_macro_step_bwd per group -> ghost
 * cotangents to the neighbours' edge cells, the stored ghosts and the action).  Nothing is fused across steps: a step costs its
 * launches (~2 + groups forward, ~3 + groups backward), which is what makes any size run; networks inside the limits above
 * are ~10 x faster through dhts_net_hybrid_rollout_*.
 * Tables: dhts_hybrid_tables in the network's own lane ids (conversions, loss samples and running means follow lane-id order),
 * EXCEPT that cells are stored GROUP-MAJOR: hyb.net.lane_off[l] is the first cell of lane l in an order where the lanes of a
 * group are contiguous (the batched operator works on the state arrays in place); lane_gpos[l] is the lane's row in that order
 * (ghost rows).  hyb.lane_capacity = vehicles a micro lane holds (any value 1 .. 1024; DHTS_FAULT_CAPACITY beyond), no limit on
 * the number of micro lanes, spawning lanes or vehicles.  n_replicas must be 1.
 *   hist   [T + 1][4][C] float32 out: (r, y, u, u_eq) of every cell before step t (row 0: the empty road)
 *   queue  [T][L] out; reward [2] out = (- sum of all queue terms, the same over the first loss_steps steps)
 *   counts [4] int32 out = (vehicles spawned or admitted, vehicles deposited, hand-off events, admission draws consumed)
 * hard != 0: an evaluation episode (hard thresholds, see dhts_net_hybrid_rollout_eval); nothing is kept for a reverse sweep.
 * _bwd: g_reward [1] or NULL (= 1) -> g_action [n_action] (gradient of reward[1]). */
typedef struct dhts_netstep_group {
    int32_t lane_pos0;   /* first row of the group in the group-major lane order */
    int32_t n_lanes;     /* lanes in the group */
    int32_t n_cells;     /* cells per lane */
    int32_t cell0;       /* first cell of the group */
    double dx;           /* cell length */
} dhts_netstep_group;
typedef struct dhts_netstep_tables {
    dhts_hybrid_tables hyb;
    const int32_t *lane_gpos;          /* [L] device: row of macro lane l in the group-major lane order (-1: micro lane) */
    const dhts_netstep_group *groups;  /* HOST pointer */
    int32_t n_groups;
    const int32_t *micro_lanes;        /* [hyb.n_micro] device: ids of the micro lanes, ascending */
    const int32_t *lane_mslot;         /* [L] device: position of lane l in micro_lanes (-1: macro lane) */
    const int32_t *cap_lanes;          /* [n_caps] device: macro lanes with a micro successor (flux capacitors), ascending */
    const int32_t *lane_cslot;         /* [L] device: position of lane l in cap_lanes (-1: none) */
    int32_t n_caps;
    const int32_t *inter_ptr, *inter_idx; /* device: ghost slots (2 lane + side) of every intersection, ascending ([sq + 1], [..]) */
    int32_t max_events;                /* capacity of the hand-off event list of an episode (0 = 8 per step) */
    /* persistent != 0: the PERSISTENT form -- one kernel per direction, one workgroup per replica, all T steps, the workgroup's
     * threads looping over the network's items with workgroup barriers where the stepwise form has kernel boundaries (same device
     * functions: same numbers).  ~30 us per step (forward + reverse) at 360 lanes / 2 124 cells against ~80 us of launches; the
     * one workgroup is the limit (beyond ~10 items per thread the stepwise form, which spreads a step over the chip, wins).
     * What fits a workgroup's LDS is kept there for the whole episode (static tables, per-step table rows, ghosts, the step's signals,
     * routes; the state rows and cotangent planes; the vehicle slots [n_micro][lane_capacity] and their cotangents): size
     * hyb.lane_capacity to the lanes (longest micro lane in vehicles + 2, dhts/stepwise.py default_lane_capacity) rather than to 32.
     * cell_lane is read by BOTH forms (the queue loss runs a thread per cell).
     * n_replicas > 1 is allowed then: action [R][A], hist [R][T + 1][4][C], queue [R][T][L], reward [R][2], counts [R][4],
     * g_reward [R], g_action [R][A]; per-replica [T][L] tables through hyb.net.replica_stride / hyb.draws_stride as in
     * dhts_net_hybrid_rollout_fwd.  cell_lane [n_cells] (device): the lane of every cell (group-major order), required whenever
     * n_cells > 0; if_lane [n_cells + ARZ lanes] (device): the lane of interface item lane_off[l] + lane_gpos[l] + k, k = 0 .. n --
     * not read by the kernels as they stand (a cell's thread solves both its interfaces), may be NULL. */
    const int32_t *if_lane, *cell_lane;
    int32_t persistent;
    int32_t n_inter_slots;             /* length of inter_idx (the persistent kernels stage the static tables in LDS) */
} dhts_netstep_tables;
size_t dhts_netstep_workspace_bytes(const dhts_net_desc *d, const dhts_netstep_tables *t);
int dhts_netstep_rollout_fwd(const dhts_net_desc *d, const dhts_netstep_tables *t, int hard, const float *action, float *hist,
                             float *queue, float *reward, int32_t *counts, void *workspace, dhts_error *err, void *stream);
int dhts_netstep_rollout_bwd(const dhts_net_desc *d, const dhts_netstep_tables *t, const float *action, const float *hist,
                             const float *queue, const float *g_reward, float *g_action, void *workspace, dhts_error *err,
                             void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DHTS_H */
