"""Hand-built macro-only road networks, one per LAUNCH LAYOUT of the network kernels (csrc/network_kernels.hip, hybrid_kernels.hip,
netstep_hybrid.hip, dhts/batched.py).  Plain numpy: no GPU, no torch.

The fused macro pair assigns thread roles from the sizes it is launched with.  With C cells, L lanes, A = n_action,
Bp = pad64(max(C + L, A)) and Cp = pad64(C) (network_kernels.hip: net_block, net_fwd_block, the two kernels' role set-up):

* forward block   Bp + Cp with wavefronts of their own for the loss where that fits 1024 threads, else Bp (loss behind the physics role);
                  launch bound 512 / 640 / 1024 by the block.  <no loss wavefronts, 512> cannot be reached: no loss wavefronts means
                  Bp + Cp > 1024, a block of at most 512 means Bp <= 512, so Cp > 512, so C > 512 -- but Bp >= pad64(C + L) > 512.  It is
                  not tested.
* reverse / evaluation block   Bp, launch bound 512 / 1024 (the evaluation kernel: 1024).
* right-hand ghost threads     start at gb1 = pad64(L) if pad64(L) + L fits the physics threads, else at L (one wavefront runs both sides).
* signal threads               start at sg_base = the block's last wavefront if sq <= 64 and the block has at least 128 threads, else at 0.

`layout()` recomputes gb1 and sg_base from these formulas, so that a case cannot silently stop reaching its branch; the block sizes
and bounds are asked of the library (dhts.ops.net_macro_plan) and compared with `Case.plan`.

Every case is built from plain arrays into a dhts.network.MacroNetworkTables and the equivalent all-macro HybridNetworkTables, with
(sq, F, dt, u_max, static_speed, vehicle_length), T <= 48 and three action vectors:

    plain   uniform(0.1, 0.9)
    edges   in every phase row entries from {0, 1, -0.25, 1.5, k / F (the progress of some frame), p + 0.5 and p - 0.5 for a frame's
            progress p (|32 (a - p)| = 16: the sigmoid's clamp edge, inclusive), the float32 neighbours of those two}
    mixed   plain with a quarter of its entries replaced from the same set

F is 8 unless the case says otherwise, so that frame / F, p +- 0.5 and a == progress are exact in float32.  All draws are seeded by
the case name (SEEDS lists the attempt that is kept).  Cell lengths 4 m and 5 m with dt = 0.1 s and u_max = 20 m/s keep every
lane inside CFL (u_max dt = 2 m); inflow schedules are uniform(0.05, 0.6).

Adjustments to the table of the issue this module answers:
* edge_65: one-cell lanes add 2 to C + L each, so 65 cannot be reached from one_wave's 62; the family's second mid lane has 3 cells
  instead of 2 (63) and one isolated lane is added.
* one_wave, edge_64, action_wide_trim, phase_clamp and the t_edges cases also take the ghost fall-back (12 lanes, one wavefront);
  `layout()` reports it.
* T = 0 is left out of t_edges: dhts.ops.net_macro_rollout sizes its tape as T * ..., an empty torch tensor's data pointer is NULL and
  dhts_net_macro_rollout_fwd answers DHTS_E_INVALID to a NULL tape (the same holds for kc and queue) -- the wrappers do not handle it,
  so nothing is launched with it.
"""
import zlib

import numpy as np

from dhts.network import SIG_ALWAYS, SIG_NS, SIG_WE, HybridNetworkTables, MacroNetworkTables

DT, U_MAX, STATIC_SPEED, VEHICLE_LENGTH = 0.1, 20.0, 0.2, 5.0

# case -> attempt whose seed is kept (seed = crc32("<case>#<attempt>")): the first attempt, counted from 0, with which the case meets
# the conditioning rule of tests/test_net_cases.py (the whole-vector ulp spread of the oracle's gradient <= 0.1 TOL_GRAD under every
# action, all the rows -- >= 90 % of at most six -- well conditioned under `plain`) and its other conditions (a gradient in two rows and
# two gating intersections, signals inside and outside the sigmoid's open range, an a == progress step under `edges`).  Every earlier
# attempt was tried and missed one of them: profiles/net_layout_cases.log lists each with what it missed.  The oracle's own float32
# arithmetic moves its gradient by about 1e-5 of the largest entry under one ulp of the action, which is why some cases took many.
SEEDS = {"one_wave": 2, "edge_64": 3, "ghost_split_fits": 130, "ghost_fallback": 61, "action_wide": 9, "sq_65": 7, "fan_4": 33, "t_edges_F1": 1,
         "bound_1024_lw": 1, "nolw_640": 2, "nolw_1024": 4}


def pad64(n):
    return (int(n) + 63) & ~63


def _seed(name):
    return zlib.crc32(("%s#%d" % (name, SEEDS.get(name, 0))).encode())


class Net:
    """Lanes and edges collected by hand."""

    def __init__(self):
        self.ncell, self.dx, self.kind, self.inter, self.edges = [], [], [], [], []

    def lane(self, n, dx, kind, inter):
        self.ncell.append(int(n)); self.dx.append(float(dx)); self.kind.append(int(kind)); self.inter.append(int(inter))
        return len(self.ncell) - 1

    def edge(self, a, b):
        self.edges.append((a, b))

    @property
    def L(self):
        return len(self.ncell)

    @property
    def C(self):
        return int(sum(self.ncell))

    def nxt(self):
        out = [[] for _ in range(self.L)]
        for a, b in self.edges:
            out[a].append(b)
        return out

    def prv(self):
        out = [[] for _ in range(self.L)]
        for a, b in self.edges:
            out[b].append(a)
        return out


class Case:
    """name, tab (MacroNetworkTables), htab (all-macro HybridNetworkTables), routes (no vehicle ever spawns: one row of -1), args =
    (sq, F, dt, u_max, static_speed, vehicle_length), T, A, actions {"plain" | "edges" | "mixed": float32 [A]}, plan (what
    dhts.ops.net_macro_plan must answer), want (the device-side choices the case was built for: subset of layout()'s keys), why."""

    def __init__(self, name, net, route, sched, sq, F, T, A, rng, plan, want, why):
        self.name, self.sq, self.F, self.T, self.A, self.plan, self.want, self.why = name, int(sq), int(F), int(T), int(A), plan, want, why
        length = [n * dx for n, dx in zip(net.ncell, net.dx)]
        self.tab = MacroNetworkTables(net.ncell, length, net.edges, net.kind, net.inter, route, sched)
        self.htab = HybridNetworkTables(np.ones(net.L, dtype=np.int32), net.ncell, length, net.edges, net.kind, net.inter, route, sched)
        self.routes = -np.ones((1, 2), dtype=np.int32)
        self.args = (self.sq, self.F, DT, U_MAX, STATIC_SPEED, VEHICLE_LENGTH)
        self.L, self.C = self.tab.n_lanes, self.tab.n_cells
        self.max_in = max(len(p) for p in net.prv())
        self.max_out = max(len(n) for n in net.nxt())
        self.n_red = int((self.tab.left_gate == -1).sum())
        self.actions = make_actions(rng, self.A, self.sq, self.F)

    # ---- what the kernels decide on the device, from the formulas in their comments ------------------------------------------------
    def layout(self):
        """{"fwd" | "bwd": {"block", "phys", "gb1", "ghost_split", "sg_base"}}: physics threads (the forward's block less its loss
        wavefronts), first right-hand ghost thread and whether the two sides sit on wavefronts of their own, first signal thread."""
        L, C, sq = self.L, self.C, self.sq
        Bp = pad64(max(C + L, self.A))
        lw = Bp + pad64(C) <= 1024
        out = {}
        for key, block, phys in (("fwd", Bp + pad64(C) if lw else Bp, Bp), ("bwd", Bp, Bp)):
            split = pad64(L) + L <= phys
            out[key] = dict(block=block, phys=phys, gb1=pad64(L) if split else L, ghost_split=split,
                            sg_base=(((block >> 6) - 1) << 6) if (sq <= 64 and block >= 128) else 0)
        return out

    def hybrid_plan(self):
        """What the fused hybrid pair takes for the all-macro tables (hybrid_kernels.hip: hyb_block, hyb_plan): block = pad64(max(C + L,
        2 L, A)) + 64 for the micro wavefront; launch bound 512 / 768 / 1024 by the block (three replicas never pack two to a unit).  The
        cases were not chosen for it: this records what they reach (test_net_cases_gpu.py asserts the block against ops.net_hybrid_plan)."""
        block = pad64(max(self.C + self.L, 2 * self.L, self.A)) + 64
        return dict(block=block, bound=512 if block <= 512 else (768 if block <= 768 else 1024))

    # ---- the structure of d reward / d action ---------------------------------------------------------------------------------------
    def rows(self):
        """Phase rows of the action vector: A // sq (a trailing remainder belongs to no row)."""
        return self.A // self.sq

    def last_row_reached(self):
        return min((self.T - 1) // self.F, self.rows() - 1)

    def structural_zeros(self):
        """bool [A]: entries whose gradient is exactly 0 for a structural reason -- rows past the last phase the episode reaches, the
        trailing entries that belong to no row, intersections that gate no lane (no signalled lane names them)."""
        z = np.zeros(self.A, dtype=bool)
        z[(self.last_row_reached() + 1) * self.sq:] = True
        gating = set(int(q) for q, k in zip(self.tab.inter, self.tab.sig_kind) if k != SIG_ALWAYS)
        for q in range(self.sq):
            if q not in gating:
                z[q:self.rows() * self.sq:self.sq] = True
        return z

    def sigmoid_range_counts(self, action):
        """(signals inside the sigmoid's open range |32 (a - progress)| < 16, signals outside or on its edge) over steps and gating
        intersections, the arithmetic of phase_signal_at in float32."""
        a = np.asarray(action, dtype=np.float32)
        inside = outside = 0
        gating = sorted(set(int(q) for q, k in zip(self.tab.inter, self.tab.sig_kind) if k != SIG_ALWAYS))
        for t in range(self.T):
            row = min(t // self.F, self.rows() - 1)
            pr = np.float32(min((t % self.F) / self.F, 1.0))
            for q in gating:
                z = (a[row * self.sq + q] - pr) * np.float32(32.0)
                if abs(z) < 16:
                    inside += 1
                else:
                    outside += 1
        return inside, outside

    def neither_light_steps(self, action):
        """Steps and gating intersections of an evaluation episode with a == progress exactly: neither light is on."""
        a = np.asarray(action, dtype=np.float32)
        n = 0
        for t in range(self.T):
            row = min(t // self.F, self.rows() - 1)
            pr = np.float32(min((t % self.F) / self.F, 1.0))
            n += int(sum(a[row * self.sq + int(q)] == pr for q, k in zip(self.tab.inter, self.tab.sig_kind) if k != SIG_ALWAYS))
        return n

    def describe(self):
        lay = self.layout()
        return ("%s: L %d C %d A %d T %d sq %d F %d | plan fwd %d (loss waves %d, bound %d) bwd %d (bound %d) | fwd gb1 %d (%s) sg_base %d | "
                "bwd gb1 %d (%s) sg_base %d | hybrid block %d bound %d | fan-in %d fan-out %d red gates %d"
                % (self.name, self.L, self.C, self.A, self.T, self.sq, self.F, self.plan["fwd_block"], self.plan["loss_waves"],
                   self.plan["fwd_bound"], self.plan["bwd_block"], self.plan["bwd_bound"], lay["fwd"]["gb1"],
                   "split" if lay["fwd"]["ghost_split"] else "one wavefront runs both sides", lay["fwd"]["sg_base"], lay["bwd"]["gb1"],
                   "split" if lay["bwd"]["ghost_split"] else "one wavefront runs both sides", lay["bwd"]["sg_base"], self.hybrid_plan()["block"],
                   self.hybrid_plan()["bound"], self.max_in,
                   self.max_out, self.n_red))


# ---- actions -------------------------------------------------------------------------------------------------------------------------
def edge_values(rng, F):
    """One draw of each kind of the edge set (float32): 0, 1, -0.25, 1.5, k / F, p + 0.5, p - 0.5 and the four float32 neighbours of the
    last two."""
    f32 = np.float32
    k = f32(int(rng.integers(0, F)) / F)
    hi, lo = f32(f32(int(rng.integers(0, F)) / F) + f32(0.5)), f32(f32(int(rng.integers(0, F)) / F) - f32(0.5))
    return [f32(0.0), f32(1.0), f32(-0.25), f32(1.5), k, hi, lo, np.nextafter(hi, f32(9)), np.nextafter(hi, f32(-9)), np.nextafter(lo, f32(9)),
            np.nextafter(lo, f32(-9))]


def make_actions(rng, A, sq, F):
    plain = rng.uniform(0.1, 0.9, A).astype(np.float32)
    edges = np.empty(A, dtype=np.float32)
    kind = 0
    for r0 in range(0, A, sq):                       # every phase row walks on through the kinds, in a shuffled order of entries
        idx = np.arange(r0, min(r0 + sq, A))
        rng.shuffle(idx)
        for i in idx:
            edges[i] = edge_values(rng, F)[kind % 11]
            kind += 1
    mixed = plain.copy()
    pick = rng.permutation(A)[:max(1, A // 4)]
    for i in pick:
        mixed[i] = edge_values(rng, F)[int(rng.integers(0, 11))]
    return dict(plain=plain, edges=edges, mixed=mixed)


# ---- topologies ----------------------------------------------------------------------------------------------------------------------
def draw_routes(rng, net, T):
    """macro_route [T][L]: every lane with successors picks one per step.  A lane with several upstream lanes must be matched every
    step (MacroNetworkTables asserts it); the generators below give such a lane upstream lanes of its own, and route_for_merge()
    overrides their picks."""
    nxt = net.nxt()
    route = -np.ones((T, net.L), dtype=np.int32)
    for t in range(T):
        for l in range(net.L):
            if nxt[l]:
                route[t, l] = nxt[l][int(rng.integers(0, len(nxt[l])))]
    return route


def schedules(rng, net, T):
    return rng.uniform(0.05, 0.6, (net.L, T))


def one_wave_net(mid2=2, isolated=0):
    """1 intersection; 4 approaching lanes (2 west-east, 2 north-south) -> 4 mid lanes -> 4 leaving lanes; lanes of 1, 8, 9 and 17 cells
    (the lane queue's eight-at-a-time loads: one clamped group, exactly one group, one group and one cell, two groups and one cell)."""
    net = Net()
    app = [net.lane(n, dx, k, 0) for n, dx, k in ((17, 5.0, SIG_WE), (9, 4.0, SIG_NS), (8, 5.0, SIG_WE), (1, 4.0, SIG_NS))]
    mid = [net.lane(n, dx, SIG_ALWAYS, 0) for n, dx in ((1, 5.0), (mid2, 4.0), (3, 5.0), (1, 5.0))]
    out = [net.lane(n, dx, SIG_ALWAYS, 0) for n, dx in ((3, 5.0), (2, 5.0), (1, 4.0), (2, 5.0))]
    for a, m, o in zip(app, mid, out):
        net.edge(a, m); net.edge(m, o)
    for i in range(isolated):                        # isolated one-cell lanes: inflow schedule on the left, their stored ghost on the right
        net.lane(1, 5.0, (SIG_ALWAYS, SIG_WE, SIG_NS)[i % 3], 0)
    return net


def units_net(rng, L, C, inters, max_cells=17):
    """L lanes with C cells of the tests' random-network kind: units of an approaching lane (signalled), one or two mid lanes behind it
    (two: the per-step route picks one, the other one's gate is red) and a leaving lane behind each; leaving lanes feed approaching lanes
    of other intersections or end; what is left over are isolated lanes.  `inters`: the intersections the units go round."""
    net = Net()
    app, leave, k = [], [], 0
    while net.L + 3 <= L:
        q = inters[k % len(inters)]
        a = net.lane(1, float(rng.choice([5.0, 4.0])), (SIG_WE, SIG_NS)[(k // len(inters)) % 2], q)
        app.append(a)
        for _ in range(2 if (net.L + 4 <= L and rng.integers(0, 2)) else 1):
            m = net.lane(1, float(rng.choice([5.0, 4.0])), SIG_ALWAYS, q)
            o = net.lane(1, 5.0, SIG_ALWAYS, q)
            net.edge(a, m); net.edge(m, o)
            leave.append(o)
        k += 1
    while net.L < L:
        net.lane(1, float(rng.choice([5.0, 4.0])), (SIG_WE, SIG_NS, SIG_ALWAYS)[net.L % 3], inters[net.L % len(inters)])
    free = list(app)
    rng.shuffle(free)
    rng.shuffle(leave)
    for o in leave[:len(leave) // 2]:
        if not free:
            break
        a = free.pop()
        if net.inter[a] != net.inter[o]:
            net.edge(o, a)
    extra = C - net.L
    assert extra >= 0
    while extra > 0:                                  # the remaining cells, one at a time onto random lanes
        l = int(rng.integers(0, net.L))
        if net.ncell[l] < max_cells:
            net.ncell[l] += 1
            extra -= 1
    return net


def fan_net():
    """Lane X with 4 upstream and 4 downstream lanes.  Upstream lanes u0..u3 (signalled, intersection 0) each also feed a side lane of
    their own; every step exactly one of them is routed into X (another one each step), the others into their side lanes -- so the side
    lane of the chosen one has nobody routed into it (left_gate = -1, red).  X picks one of d0..d3 per step (the others are red); d0 and d1
    are the approaching lanes of intersection 1 with a leaving lane each, d2, d3 and the side lanes are sinks (stored ghosts)."""
    net = Net()
    ups = [net.lane(n, dx, k, 0) for n, dx, k in ((3, 5.0, SIG_WE), (1, 4.0, SIG_NS), (2, 5.0, SIG_WE), (9, 4.0, SIG_NS))]
    x = net.lane(4, 5.0, SIG_ALWAYS, 0)
    side = [net.lane(n, 5.0, SIG_ALWAYS, 0) for n in (1, 2, 1, 3)]
    downs = [net.lane(n, dx, k, 1) for n, dx, k in ((2, 5.0, SIG_WE), (1, 4.0, SIG_NS), (1, 5.0, SIG_ALWAYS), (8, 4.0, SIG_ALWAYS))]
    outs = [net.lane(n, 5.0, SIG_ALWAYS, 1) for n in (2, 1)]
    for u, s in zip(ups, side):
        net.edge(u, x); net.edge(u, s)
    for d in downs:
        net.edge(x, d)
    net.edge(downs[0], outs[0]); net.edge(downs[1], outs[1])
    return net, ups, x, side, downs


def fan_routes(rng, net, T, ups, x, side, downs):
    route = draw_routes(rng, net, T)
    chosen = 0
    for t in range(T):
        chosen = (chosen + 1 + int(rng.integers(0, 3))) % 4          # never the same upstream lane twice in a row
        for i, (u, s) in enumerate(zip(ups, side)):
            route[t, u] = x if i == chosen else s
        route[t, x] = downs[(3 * t + int(rng.integers(0, 2))) % 4]
    return route


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
def _plan(C, L, A):
    """The plan the issue's table names for a shape, from the arithmetic in the module docstring (asserted against the library)."""
    Bp = pad64(max(C + L, A))
    lw = Bp + pad64(C) <= 1024
    fb = Bp + pad64(C) if lw else Bp
    return dict(fwd_block=fb, loss_waves=lw, fwd_bound=512 if fb <= 512 else (640 if fb <= 640 else 1024), bwd_block=Bp,
                bwd_bound=512 if Bp <= 512 else 1024)


def _rows_used(T, F):
    return (T + F - 1) // F


def _simple(name, net, sq, F, T, A, plan, want, why, routes=None):
    rng = np.random.default_rng(_seed(name))
    route = routes(rng, net, T) if routes else draw_routes(rng, net, T)
    sched = schedules(rng, net, T)
    got = _plan(net.C, net.L, A)
    assert got == plan, "%s: the shape gives plan %s, the case names %s" % (name, got, plan)
    return Case(name, net, route, sched, sq, F, T, A, rng, plan, want, why)


def _p(fb, lw, fbound, bb, bbound):
    return dict(fwd_block=fb, loss_waves=lw, fwd_bound=fbound, bwd_block=bb, bwd_bound=bbound)


def _units(name, L, C, inters):
    return units_net(np.random.default_rng(_seed(name) ^ 0x5bd1e995), L, C, inters)


BUILDERS = {
    "one_wave": lambda n: _simple(n, one_wave_net(), 1, 8, 40, 5, _p(128, True, 512, 64, 512),
                                  dict(bwd=dict(block=64, sg_base=0), fwd=dict(block=128, sg_base=64)),
                                  "reverse and evaluation kernels at 64 threads, every role in one wavefront; forward at 128; queue loads at 1, 8, 9, 17 cells"),
    "edge_64": lambda n: _simple(n, one_wave_net(isolated=1), 1, 8, 40, 5, _p(128, True, 512, 64, 512),
                                 dict(bwd=dict(block=64, sg_base=0)), "C + L = 64: the last shape of the 64-thread block"),
    "edge_65": lambda n: _simple(n, one_wave_net(mid2=3, isolated=1), 1, 8, 40, 5, _p(192, True, 512, 128, 512),
                                 dict(bwd=dict(block=128, sg_base=64)), "C + L = 65: the first shape of the 128-thread block"),
    "ghost_split_fits": lambda n: _simple(n, _units(n, 64, 64, [0, 1]), 2, 8, 40, 10, _p(192, True, 512, 128, 512),
                                          dict(bwd=dict(gb1=64, ghost_split=True, phys=128), fwd=dict(gb1=64, ghost_split=True, phys=128)),
                                          "pad64(L) + L == physics threads exactly: the split ghost layout at its limit"),
    "ghost_fallback": lambda n: _simple(n, _units(n, 65, 65, [0, 1]), 2, 8, 40, 10, _p(320, True, 512, 192, 512),
                                        dict(bwd=dict(gb1=65, ghost_split=False, phys=192), fwd=dict(gb1=65, ghost_split=False, phys=192)),
                                        "pad64(L) + L = 193 > 192: right ghosts start at thread L, one wavefront runs both sides"),
    "action_wide": lambda n: _simple(n, one_wave_net(), 2, 8, 44, 130, _p(256, True, 512, 192, 512),
                                     dict(bwd=dict(block=192, sg_base=128)), "block sized by the action count (65 phase rows, 6 used)"),
    "phase_clamp": lambda n: _simple(n, _units(n, 14, 40, [0, 1]), 2, 8, 40, 5, _p(128, True, 512, 64, 512), dict(),
                                     "T = 5 F with 2 phase rows: steps past the last row reuse it; A = 2 sq + 1: the odd entry has gradient 0"),
    "sq_65": lambda n: _simple(n, _units(n, 30, 70, [0, 63, 64]), 65, 8, 24, 130, _p(320, True, 512, 192, 512),
                               dict(bwd=dict(sg_base=0), fwd=dict(sg_base=0)), "sq > 64: signal threads are [0, sq); 62 intersections gate no lane"),
    "fan_4": lambda n: (lambda f: _simple(n, f[0], 2, 8, 40, 10, _p(128, True, 512, 64, 512), dict(),
                                          "4 upstream and 4 downstream lanes, the route changing every step; red gates; sinks",
                                          routes=lambda rng, net, T: fan_routes(rng, net, T, *f[1:])))(fan_net()),
    "t_edges_T1": lambda n: _simple(n, one_wave_net(), 1, 8, 1, 2, _p(128, True, 512, 64, 512), dict(), "T = 1: both step-ahead fetches clamp at once"),
    "t_edges_T7": lambda n: _simple(n, one_wave_net(), 1, 8, 7, 2, _p(128, True, 512, 64, 512), dict(), "T = F - 1: the phase counter never wraps"),
    "t_edges_T11": lambda n: _simple(n, one_wave_net(), 1, 8, 11, 2, _p(128, True, 512, 64, 512), dict(), "T = F + 3: one wrap, a short second phase"),
    "t_edges_F1": lambda n: _simple(n, one_wave_net(), 1, 1, 40, 32, _p(128, True, 512, 64, 512), dict(),
                                    "F = 1: a phase per step, progress always 0; the last eight steps reuse the last row"),
    "bound_512": lambda n: _simple(n, _units(n, 50, 200, [0, 1, 2, 3]), 4, 8, 32, 16, _p(512, True, 512, 256, 512), dict(), "forward <loss waves, 512>; reverse 512"),
    "bound_640": lambda n: _simple(n, _units(n, 60, 250, [0, 1, 2, 3]), 4, 8, 32, 16, _p(576, True, 640, 320, 512), dict(), "forward <loss waves, 640>"),
    "bound_1024_lw": lambda n: _simple(n, _units(n, 100, 448, [0, 1, 2, 3]), 4, 8, 24, 12, _p(1024, True, 1024, 576, 1024), dict(),
                                       "forward <loss waves, 1024> at the full workgroup; reverse 1024"),
    "nolw_640": lambda n: _simple(n, _units(n, 100, 500, [0, 1, 2, 3]), 4, 8, 24, 12, _p(640, False, 640, 640, 1024), dict(),
                                  "forward without loss wavefronts, 640 threads"),
    "nolw_1024": lambda n: _simple(n, _units(n, 130, 520, [0, 1, 2, 3]), 4, 8, 24, 12, _p(704, False, 1024, 704, 1024), dict(),
                                   "forward without loss wavefronts, 704 threads, bound 1024"),
}
NAMES = list(BUILDERS) + ["action_wide_trim"]
_CACHE = {}


def case(name):
    """The named case (built once per process)."""
    if name not in _CACHE:
        if name == "action_wide_trim":              # the twin: the same network and episode, A cut to the rows the episode uses
            w = case("action_wide")
            c = Case.__new__(Case)
            c.__dict__.update(w.__dict__)
            c.name, c.A = name, w.sq * _rows_used(w.T, w.F)
            c.actions = {k: v[:c.A].copy() for k, v in w.actions.items()}
            c.plan = _p(128, True, 512, 64, 512)
            assert _plan(c.C, c.L, c.A) == c.plan
            c.want = dict(bwd=dict(block=64, sg_base=0))
            c.why = "action_wide with A cut to the 6 rows the episode uses: block 64"
            _CACHE[name] = c
        else:
            _CACHE[name] = BUILDERS[name](name)
        c = _CACHE[name]
        lay = c.layout()
        for side, want in c.want.items():
            for k, v in want.items():
                assert lay[side][k] == v, "%s: %s %s is %s, the case was built for %s" % (name, side, k, lay[side][k], v)
    return _CACHE[name]


# ---- the reference: the CPU oracle's episodes of a case, and how far its own gradient moves under one ulp of the action ---------------
WELL = 0.1 * 1e-4            # 0.1 TOL_GRAD: the ulp spread below which the whole vector / a phase row is well conditioned
_REF = {}


def _ulp(a, up):
    return np.nextafter(np.asarray(a, dtype=np.float32), np.float32(np.inf if up else -np.inf))


def reference(name, oracle):
    """{action name: dict(train = oracle.net_macro(...), hard = the evaluation episode, spread = the whole-vector ulp spread of
    g_action (max |g(a +- 1 ulp) - g(a)| / max |g|), row_max [rows] = each phase row's largest |g|, row_spread [rows] = each row's
    largest move relative to row_max (0 where the row's gradient is 0), well [rows] = rows with a non-zero gradient whose spread is at most
    0.1 TOL_GRAD)}, computed once per process."""
    if name in _REF:
        return _REF[name]
    c = case(name)
    out = {}
    for an, a in c.actions.items():
        o = oracle.net_macro(c.tab, a, *c.args)
        g = o["g_action"].astype(np.float64)
        moved = np.zeros_like(g)
        for up in (True, False):
            moved = np.maximum(moved, np.abs(oracle.net_macro(c.tab, _ulp(a, up), *c.args)["g_action"].astype(np.float64) - g))
        R, sq = c.rows(), c.sq
        row_max = np.abs(g[:R * sq]).reshape(R, sq).max(axis=1)
        row_move = moved[:R * sq].reshape(R, sq).max(axis=1)
        row_spread = np.where(row_max > 0, row_move / np.maximum(row_max, 1e-300), 0.0)
        out[an] = dict(train=o, hard=oracle.net_macro(c.tab, a, *c.args, hard=True), spread=float(moved.max() / max(np.abs(g).max(), 1e-300)),
                       row_max=row_max, row_spread=row_spread, well=(row_max > 0) & (row_spread <= WELL))
    _REF[name] = out
    return out


def conditioning_failures(name, oracle):
    """The conditioning rule, as a list of what misses it (empty: the case's seed stands)."""
    bad = []
    ref = reference(name, oracle)
    for an, r in ref.items():
        if r["spread"] > WELL:
            bad.append("%s: whole-vector spread %.2e" % (an, r["spread"]))
    nz = ref["plain"]["row_max"] > 0
    if nz.any() and ref["plain"]["well"].sum() < 0.9 * nz.sum():
        bad.append("plain: %d of %d rows well conditioned" % (ref["plain"]["well"].sum(), nz.sum()))
    return bad


def nontrivial_failures(name, oracle):
    """The conditions on a case's gradient and signals, as a list of what misses them: under `plain` two phase rows carry gradient
    (where the episode reaches two) and two gating intersections (where the case has two); in episodes of at least 8 steps every action
    has signals inside and outside the sigmoid's open range, and `edges` has a step with a == progress."""
    c, ref, bad = case(name), reference(name, oracle), []
    g = np.abs(ref["plain"]["train"]["g_action"][:c.rows() * c.sq]).reshape(c.rows(), c.sq)
    gating = set(int(q) for q, k in zip(c.tab.inter, c.tab.sig_kind) if k != SIG_ALWAYS)
    if c.last_row_reached() >= 1:
        if (g.max(axis=1) > 0).sum() < 2:
            bad.append("plain: fewer than 2 rows with gradient")
        if len(gating) >= 2 and (g.max(axis=0) > 0).sum() < 2:
            bad.append("plain: fewer than 2 intersections with gradient")
    if c.T >= 8:
        for an, a in c.actions.items():
            inside, outside = c.sigmoid_range_counts(a)
            if inside == 0 or outside == 0:
                bad.append("%s: signals inside the open range %d, outside %d" % (an, inside, outside))
        if c.neither_light_steps(c.actions["edges"]) == 0:
            bad.append("edges: no step with a == progress")
    return bad


def try_seeds(name, oracle, limit=400):
    """(attempt kept, [(attempt, what it missed)]): the first attempt at which the case meets conditioning_failures and
    nontrivial_failures, trying from 0 (tools/probes/net_case_seeds.py prints this for profiles/net_layout_cases.log)."""
    if name == "action_wide_trim":
        raise ValueError("action_wide_trim is cut from action_wide")
    keep, tried = SEEDS.get(name, 0), []
    try:
        for k in range(limit):
            SEEDS[name] = k
            _CACHE.pop(name, None); _REF.pop(name, None)
            bad = conditioning_failures(name, oracle) + nontrivial_failures(name, oracle)
            if any(r[m]["rc"] != 0 for r in reference(name, oracle).values() for m in ("train", "hard")):
                bad.append("CFL fault")
            if not bad:
                return k, tried
            tried.append((k, bad))
        return None, tried
    finally:
        SEEDS[name] = keep
        if keep == 0:
            del SEEDS[name]
        _CACHE.pop(name, None); _REF.pop(name, None)
