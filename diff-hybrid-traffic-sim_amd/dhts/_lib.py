"""ctypes binding of libdhts.so (C ABI: include/dhts.h).

The shared object is built in-tree by `diff-hybrid-traffic-sim_amd/csrc/Makefile` (driven by
`__graft_entry__.build()`).  There is NO fallback: if the library is missing or a call fails, an exception
is raised -- the product path never routes through a CPU implementation.
"""
import ctypes as C
import operator
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(_HERE), "csrc")
# DHTS_LIB: another build of the same library (tuning experiments: tools/build_variants.sh); the default is the in-tree build
SO_PATH = os.environ.get("DHTS_LIB") or os.path.join(CSRC, "libdhts.so")

OK, E_INVALID, E_LAUNCH, E_NO_DEVICE = 0, -1, -2, -3
FAULT_NONE, FAULT_CFL, FAULT_COLLISION, FAULT_NAN, FAULT_CAPACITY = 0, 1, 2, 3, 4
OPT_MACRO_FWD_WAVES = 1
OPT_MICRO_FWD_WAVES = 2
OPT_MACRO_FWD_VARIANT = 3
OPT_MACRO_FWD_GROUP = 4
OPT_MACRO_FWD_ROTATE = 5
OPT_NETSTEP_LDS_KB = 6
OPT_NETSTEP_BLOCK = 7
OPT_HYB_PACK = 8
OPT_REWARD_CHAIN = 9
OPT_MACRO_JVP_VARIANT = 11
MACRO_MAX_CELLS = 4000
MICRO_MAX_VEHICLES = 1024


class MacroDesc(C.Structure):
    _fields_ = [("n_lanes", C.c_int32), ("n_cells", C.c_int32), ("dt", C.c_double), ("dx", C.c_double),
                ("u_max", C.c_double)]


class NetDesc(C.Structure):
    _fields_ = [("n_replicas", C.c_int32), ("n_lanes", C.c_int32), ("n_cells", C.c_int32), ("n_steps", C.c_int32),
                ("n_inter_sq", C.c_int32), ("frames_per_phase", C.c_int32), ("n_action", C.c_int32),
                ("dt", C.c_double), ("u_max", C.c_double), ("static_speed", C.c_double), ("vehicle_length", C.c_double)]


class NetTables(C.Structure):
    _fields_ = [("lane_ncell", C.c_void_p), ("lane_off", C.c_void_p), ("sig_kind", C.c_void_p), ("inter", C.c_void_p),
                ("lane_dx", C.c_void_p), ("left_src", C.c_void_p), ("left_gate", C.c_void_p), ("right_src", C.c_void_p),
                ("schedule", C.c_void_p), ("replica_stride", C.c_int64), ("nxt_ptr", C.c_void_p), ("nxt_idx", C.c_void_p),
                ("prv_ptr", C.c_void_p), ("prv_idx", C.c_void_p), ("n_edges", C.c_int32)]


class HybridTables(C.Structure):
    _fields_ = [("net", NetTables), ("lane_macro", C.c_void_p), ("lane_len", C.c_void_p), ("conv_next", C.c_void_p),
                ("routes", C.c_void_p), ("route_ptr", C.c_void_p), ("n_routes", C.c_int32), ("route_stride", C.c_int32),
                ("records_per_step", C.c_int32), ("loss_steps", C.c_int32), ("n_micro", C.c_int32),
                ("lane_source", C.c_void_p), ("draws", C.c_void_p), ("n_draws", C.c_int32), ("draws_stride", C.c_int64),
                ("lane_capacity", C.c_int32), ("micro_tensor_ladder", C.c_int32), ("veh_params", C.c_void_p), ("two_per_cu", C.c_int32)]


class HybridStateIO(C.Structure):
    _fields_ = [("plain", C.c_int32), ("state0", C.c_void_p), ("ghost0", C.c_void_p), ("veh_out", C.c_void_p), ("events", C.c_void_p)]


class NetstepGroup(C.Structure):
    _fields_ = [("lane_pos0", C.c_int32), ("n_lanes", C.c_int32), ("n_cells", C.c_int32), ("cell0", C.c_int32), ("dx", C.c_double)]


class NetstepTables(C.Structure):
    _fields_ = [("hyb", HybridTables), ("lane_gpos", C.c_void_p), ("groups", C.POINTER(NetstepGroup)), ("n_groups", C.c_int32),
                ("micro_lanes", C.c_void_p), ("lane_mslot", C.c_void_p), ("cap_lanes", C.c_void_p), ("lane_cslot", C.c_void_p),
                ("n_caps", C.c_int32), ("inter_ptr", C.c_void_p), ("inter_idx", C.c_void_p), ("max_events", C.c_int32),
                ("if_lane", C.c_void_p), ("cell_lane", C.c_void_p), ("persistent", C.c_int32), ("n_inter_slots", C.c_int32)]


class MicroDesc(C.Structure):
    _fields_ = [("n_lanes", C.c_int32), ("capacity", C.c_int32), ("dt", C.c_double)]


# ---- the one description of the C ABI: every symbol include/dhts.h declares, its parameters in the header's names and order ----
# A word is a parameter.  A bare word is a pointer the library takes as `void *` (float / double / int32_t arrays, dhts_error, the
# stream); `name:code` is anything else: i = int (and the by-value int32_t), i64 = int64_t, f64 = double, i32x8 = int32_t plan[8],
# i32p = int32_t *, a struct's name = a const pointer to it.  The functions return int (a DHTS_E_* status) unless the entry starts
# with "size_t =".  tests/test_binding_table.py holds names, order and types to the header.
_TABLE = {
    "dhts_version": "",
    "dhts_device_count": "",
    "dhts_set_option": "option:i value:i",
    "dhts_padded": "n:i",
    "dhts_macro_tape_bytes": "size_t = d:MacroDesc T:i",
    "dhts_macro_tape_expand": "d:MacroDesc T:i tape dqs_out stream",
    "dhts_macro_step_tape_bytes": "size_t = d:MacroDesc",
    "dhts_arz_interface_batch": "n:i64 variant:i in dt:f64 dx:f64 case_ind q0 flux dL dR fp A B cfl_bad speed stream",
    "dhts_macro_state_from_ru": "n:i64 u_max:f64 r u y ueq stream",
    "dhts_macro_state_from_ru_bwd": "n:i64 u_max:f64 r u g_y g_r g_u stream",
    "dhts_macro_u_tap_bwd": "n:i64 u_max:f64 r y g_u g_r g_y stream",
    "dhts_macro_rollout_fwd": "d:MacroDesc T:i r y u ueq ghost r_out y_out u_out ueq_out tape hist err stream",
    "dhts_macro_rollout_bwd": "d:MacroDesc T:i tape g_r g_y g_hist g_r_out g_y_out g_ghost err stream",
    "dhts_macro_rollout_fwd_sched": "d:MacroDesc T:i r y u ueq ghost_sched r_out y_out u_out ueq_out tape hist err stream",
    "dhts_macro_rollout_bwd_sched": "d:MacroDesc T:i tape g_r g_y g_hist g_r_out g_y_out g_ghost_sched err stream",
    "dhts_macro_rollout_plan": "d:MacroDesc T:i want_hist:i plan:i32x8",
    "dhts_macro_rollout_fwd_taps": "d:MacroDesc T:i r y u ueq ghost ghost_is_sched:i r_out y_out u_out ueq_out tape det n_det:i "
                                   "taps err stream",
    "dhts_macro_rollout_bwd_taps": "d:MacroDesc T:i tape g_r g_y det n_det:i g_taps g_r_out g_y_out g_ghost ghost_is_sched:i err "
                                   "stream",
    "dhts_macro_taps_plan": "d:MacroDesc T:i n_det:i plan:i32x8",
    "dhts_macro_rollout_jvp": "d:MacroDesc T:i tape n_dir:i t_r t_y t_ghost ghost_is_sched:i t_r_out t_y_out det n_det:i t_taps "
                              "err stream",
    "dhts_macro_jvp_plan": "d:MacroDesc T:i n_dir:i n_det:i plan:i32x8",
    "dhts_macro_rollout_fwd_jvp": "d:MacroDesc T:i n_dir:i r y u ueq ghost ghost_is_sched:i t_r t_y t_ghost r_out y_out u_out "
                                  "ueq_out t_r_out t_y_out det n_det:i taps t_taps err err_jvp stream",
    "dhts_macro_fwd_jvp_plan": "d:MacroDesc T:i n_dir:i n_det:i plan:i32x8",
    "dhts_macro_ckpt_plan": "d:MacroDesc T:i n_det:i segment:i plan:i32x8",
    "dhts_macro_ckpt_bytes": "size_t = d:MacroDesc T:i segment:i",
    "dhts_macro_rollout_fwd_ckpt": "d:MacroDesc T:i segment:i r y u ueq ghost ghost_is_sched:i r_out y_out u_out ueq_out det "
                                   "n_det:i taps ckpt err stream",
    "dhts_macro_rollout_bwd_ckpt": "d:MacroDesc T:i segment:i ckpt r y u ueq ghost ghost_is_sched:i g_r g_y det n_det:i g_taps "
                                   "g_r_out g_y_out g_ghost err stream",
    "dhts_macro_ckpt_target_plan": "d:MacroDesc T:i segment:i plan:i32x8",
    "dhts_macro_rollout_fwd_ckpt_target": "d:MacroDesc T:i segment:i r y u ueq ghost ghost_is_sched:i r_out y_out u_out ueq_out "
                                          "ckpt target sse err stream",
    "dhts_macro_rollout_bwd_ckpt_target": "d:MacroDesc T:i segment:i ckpt r y u ueq ghost ghost_is_sched:i g_r g_y target g_sse "
                                          "r_fin y_fin u_fin g_r_out g_y_out g_ghost err stream",
    "dhts_macro_rollout_fwd_ckpt_ring": "d:MacroDesc T:i segment:i r y u ueq r_out y_out u_out ueq_out det n_det:i taps ckpt err "
                                        "stream",
    "dhts_macro_rollout_bwd_ckpt_ring": "d:MacroDesc T:i segment:i ckpt r y u ueq g_r g_y det n_det:i g_taps g_r_out g_y_out err "
                                        "stream",
    "dhts_macro_rollout_fwd_ckpt_target_ring": "d:MacroDesc T:i segment:i r y u ueq r_out y_out u_out ueq_out ckpt target sse err "
                                               "stream",
    "dhts_macro_rollout_bwd_ckpt_target_ring": "d:MacroDesc T:i segment:i ckpt r y u ueq g_r g_y target g_sse r_fin y_fin u_fin "
                                               "g_r_out g_y_out err stream",
    "dhts_macro_rollout_fwd_jvp_ring": "d:MacroDesc T:i n_dir:i r y u ueq t_r t_y r_out y_out u_out ueq_out t_r_out t_y_out det "
                                       "n_det:i taps t_taps err err_jvp stream",
    "dhts_macro_rollout_fwd_ckpt_ramp": "d:MacroDesc T:i segment:i r y u ueq ghost ghost_is_sched:i r_out y_out u_out ueq_out det "
                                        "n_det:i taps ckpt ramps n_ramp:i inflow ring:i err stream",
    "dhts_macro_rollout_bwd_ckpt_ramp": "d:MacroDesc T:i segment:i ckpt r y u ueq ghost ghost_is_sched:i g_r g_y det n_det:i "
                                        "g_taps g_r_out g_y_out g_ghost ramps n_ramp:i inflow g_inflow ring:i err stream",
    "dhts_macro_rollout_fwd_ckpt_target_ramp": "d:MacroDesc T:i segment:i r y u ueq ghost ghost_is_sched:i r_out y_out u_out "
                                               "ueq_out ckpt target sse ramps n_ramp:i inflow ring:i err stream",
    "dhts_macro_rollout_bwd_ckpt_target_ramp": "d:MacroDesc T:i segment:i ckpt r y u ueq ghost ghost_is_sched:i g_r g_y target "
                                               "g_sse r_fin y_fin u_fin g_r_out g_y_out g_ghost ramps n_ramp:i inflow g_inflow "
                                               "ring:i err stream",
    "dhts_macro_rollout_fwd_jvp_ramp": "d:MacroDesc T:i n_dir:i r y u ueq ghost ghost_is_sched:i t_r t_y t_ghost r_out y_out "
                                       "u_out ueq_out t_r_out t_y_out det n_det:i taps t_taps err err_jvp stream ramps n_ramp:i "
                                       "inflow t_inflow",
    "dhts_macro_rollout_fwd_jvp_ring_ramp": "d:MacroDesc T:i n_dir:i r y u ueq t_r t_y r_out y_out u_out ueq_out t_r_out t_y_out "
                                            "det n_det:i taps t_taps err err_jvp stream ramps n_ramp:i inflow t_inflow",
    "dhts_macro_state_from_ru_jvp": "n:i64 u_max:f64 r u t_r t_u t_y stream",
    "dhts_macro_u_tap_jvp": "n:i64 u_max:f64 r y t_r t_y t_u stream",
    "dhts_macro_step_fwd": "d:MacroDesc r y u ueq ghost r_out y_out u_out ueq_out tape err stream",
    "dhts_macro_step_bwd": "d:MacroDesc tape g_r g_y g_r_out g_y_out g_ghost err stream",
    "dhts_micro_tape_bytes": "size_t = d:MicroDesc T:i",
    "dhts_micro_step_tape_bytes": "size_t = d:MicroDesc",
    "dhts_idm_batch": "n:i64 variant:i in next_pv dEgo dLeading collided acc_sstar clips stream",
    "dhts_idm_jac_batch": "n:i64 in dEgo dLeading stream",
    "dhts_micro_rollout_fwd": "d:MicroDesc T:i p v count params head p_out v_out tape hist err stream",
    "dhts_micro_rollout_bwd": "d:MicroDesc T:i tape count g_p g_v g_hist g_p_out g_v_out g_head err stream",
    "dhts_micro_param_tape_bytes": "size_t = d:MicroDesc T:i",
    "dhts_micro_rollout_fwd_params": "d:MicroDesc T:i p v count params head p_out v_out tape ptape hist err stream",
    "dhts_micro_rollout_bwd_params": "d:MicroDesc T:i tape ptape count params g_p g_v g_hist g_p_out g_v_out g_head g_params err "
                                     "stream",
    "dhts_idm_param_jac_batch": "n:i64 in dacc clips stream",
    "dhts_micro_rollout_plan": "d:MicroDesc T:i has_count:i plan:i32x8",
    "dhts_micro_rollout_jvp": "d:MicroDesc T:i n_dir:i tape ptape count params t_p t_v t_head t_params t_p_out t_v_out t_hist err "
                              "stream",
    "dhts_micro_jvp_plan": "d:MicroDesc T:i n_dir:i want_params:i plan:i32x8",
    "dhts_micro_rollout_fwd_jvp": "d:MicroDesc T:i n_dir:i p v count params head t_p t_v t_head t_params p_out v_out t_p_out "
                                  "t_v_out hist t_hist err err_jvp stream",
    "dhts_micro_fwd_jvp_plan": "d:MicroDesc T:i n_dir:i want_params:i plan:i32x8",
    "dhts_micro_ckpt_plan": "d:MicroDesc T:i want_params:i segment:i plan:i32x8",
    "dhts_micro_ckpt_bytes": "size_t = d:MicroDesc T:i segment:i",
    "dhts_micro_rollout_fwd_ckpt": "d:MicroDesc T:i segment:i p v count params head p_out v_out ckpt hist err stream",
    "dhts_micro_rollout_bwd_ckpt": "d:MicroDesc T:i segment:i ckpt count params head g_p g_v g_hist g_p_out g_v_out g_head "
                                   "g_params err stream",
    "dhts_micro_rollout_fwd_ckpt_samples": "d:MicroDesc T:i segment:i p v count params head p_out v_out ckpt probes n_probes:i "
                                           "every:i samples err stream",
    "dhts_micro_rollout_bwd_ckpt_samples": "d:MicroDesc T:i segment:i ckpt count params head g_p g_v probes n_probes:i every:i "
                                           "g_samples g_p_out g_v_out g_head g_params err stream",
    "dhts_micro_rollout_fwd_jvp_samples": "d:MicroDesc T:i n_dir:i p v count params head t_p t_v t_head t_params p_out v_out "
                                          "t_p_out t_v_out probes n_probes:i every:i samples t_samples err err_jvp stream",
    "dhts_micro_rollout_fwd_ckpt_lead": "d:MicroDesc T:i segment:i p v count params lead lead_length p_out v_out ckpt probes "
                                        "n_probes:i every:i samples err stream",
    "dhts_micro_rollout_bwd_ckpt_lead": "d:MicroDesc T:i segment:i ckpt count params lead lead_length g_p g_v probes n_probes:i "
                                        "every:i g_samples g_p_out g_v_out g_lead g_params err stream",
    "dhts_micro_rollout_fwd_jvp_lead": "d:MicroDesc T:i n_dir:i p v count params lead lead_length t_p t_v t_lead t_params p_out "
                                       "v_out t_p_out t_v_out probes n_probes:i every:i samples t_samples err err_jvp stream",
    "dhts_micro_ckpt_target_plan": "d:MicroDesc T:i want_params:i segment:i plan:i32x8",
    "dhts_micro_rollout_fwd_ckpt_target": "d:MicroDesc T:i segment:i p v count params head lead lead_length p_out v_out ckpt "
                                          "target sse err stream",
    "dhts_micro_rollout_bwd_ckpt_target": "d:MicroDesc T:i segment:i ckpt count params head lead lead_length g_p g_v target g_sse "
                                          "g_p_out g_v_out g_head g_lead g_params err stream",
    "dhts_micro_rollout_fwd_ckpt_ring": "d:MicroDesc T:i segment:i p v count params ring p_out v_out ckpt probes n_probes:i "
                                        "every:i samples err stream",
    "dhts_micro_rollout_bwd_ckpt_ring": "d:MicroDesc T:i segment:i ckpt count params ring g_p g_v probes n_probes:i every:i "
                                        "g_samples g_p_out g_v_out g_params err stream",
    "dhts_micro_rollout_fwd_jvp_ring": "d:MicroDesc T:i n_dir:i p v count params ring t_p t_v t_params p_out v_out t_p_out "
                                       "t_v_out probes n_probes:i every:i samples t_samples err err_jvp stream",
    "dhts_micro_rollout_fwd_ckpt_target_ring": "d:MicroDesc T:i segment:i p v count params ring p_out v_out ckpt target sse err "
                                               "stream",
    "dhts_micro_rollout_bwd_ckpt_target_ring": "d:MicroDesc T:i segment:i ckpt count params ring g_p g_v target g_sse g_p_out "
                                               "g_v_out g_params err stream",
    "dhts_micro_rollout_fwd_jvp_gn": "d:MicroDesc T:i n_dir:i p v count params head lead lead_length ring t_p t_v t_head t_lead "
                                     "t_params p_out v_out t_p_out t_v_out probes n_probes:i every:i target sse jtr jtj err "
                                     "err_jvp stream",
    "dhts_micro_fwd_jvp_gn_plan": "d:MicroDesc T:i n_dir:i want_params:i plan:i32x8",
    "dhts_micro_step_fwd": "d:MicroDesc p v count params head p_out v_out tape err stream",
    "dhts_micro_step_fwd_tensor": "d:MicroDesc p v count params head p_out v_out tape err stream",
    "dhts_micro_step_fwd_tensor_head": "d:MicroDesc p v count params head p_out v_out tape err stream",
    "dhts_micro_step_bwd": "d:MicroDesc tape count g_p g_v g_p_out g_v_out g_head err stream",
    "dhts_net_macro_hist_bytes": "size_t = d:NetDesc",
    "dhts_net_macro_tape_bytes": "size_t = d:NetDesc",
    "dhts_net_macro_plan": "d:NetDesc plan:i32x8",
    "dhts_net_macro_rollout_fwd": "d:NetDesc t:NetTables action hist tape kc queue reward workspace err stream",
    "dhts_net_macro_rollout_eval": "d:NetDesc t:NetTables action queue reward err stream",
    "dhts_net_macro_rollout_bwd": "d:NetDesc t:NetTables action hist tape kc queue g_reward g_action workspace err stream",
    "dhts_net_ghosts_fwd": "d:NetDesc t:NetTables step:i hard:i action r u own_in own_out ghost stream",
    "dhts_net_ghosts_bwd": "d:NetDesc t:NetTables inter_ptr inter_idx step:i action r y u own_in g_ghost g_own_in g_own_out g_r "
                           "g_y g_action scratch stream",
    "dhts_net_hybrid_workspace_bytes": "size_t = d:NetDesc t:HybridTables",
    "dhts_net_hybrid_plan": "d:NetDesc t:HybridTables plan:i32p",
    "dhts_net_hybrid_tape_bytes": "size_t = d:NetDesc",
    "dhts_net_hybrid_rollout_fwd": "d:NetDesc t:HybridTables action hist tape kc queue reward counts workspace err stream",
    "dhts_net_hybrid_rollout_eval": "d:NetDesc t:HybridTables action queue reward counts err stream",
    "dhts_net_hybrid_rollout_bwd": "d:NetDesc t:HybridTables action hist tape kc queue g_reward g_action workspace err stream",
    "dhts_net_hybrid_state_rollout_fwd": "d:NetDesc t:HybridTables io:HybridStateIO action hist tape kc queue reward counts "
                                         "workspace err stream",
    "dhts_net_hybrid_state_rollout_bwd": "d:NetDesc t:HybridTables plain:i action hist tape kc queue g_reward g_stateT g_veh "
                                         "g_action g_state0 workspace err stream",
    "dhts_netstep_workspace_bytes": "size_t = d:NetDesc t:NetstepTables",
    "dhts_netstep_rollout_fwd": "d:NetDesc t:NetstepTables hard:i action hist queue reward counts workspace err stream",
    "dhts_netstep_rollout_bwd": "d:NetDesc t:NetstepTables action hist queue g_reward g_action workspace err stream",
}

_CODES = {"i": C.c_int, "i64": C.c_int64, "f64": C.c_double, "i32x8": C.POINTER(C.c_int32 * 8), "i32p": C.POINTER(C.c_int32)}
_CODES.update((s.__name__, C.POINTER(s)) for s in (MacroDesc, MicroDesc, NetDesc, NetTables, HybridTables, HybridStateIO, NetstepTables))


def _parse(spec):
    """An entry of _TABLE -> (restype, ((parameter name, ctypes type), ...))."""
    ret, _, words = spec.rpartition("=")
    pairs = (w.partition(":") for w in words.split())
    return (C.c_size_t if ret else C.c_int), tuple((n, _CODES[code] if code else C.c_void_p) for n, _, code in pairs)


# name -> (restype, ((parameter name, type), ...)), and what ctypes wants of it: name -> (restype, [types])
PARAMETERS = {name: _parse(spec) for name, spec in _TABLE.items()}
SIGNATURES = {name: (res, [t for _, t in params]) for name, (res, params) in PARAMETERS.items()}

_lib = None
_entries = {}        # name -> (the bound function, its parameter names, mapping -> the values in that order), made when the library is loaded


class DhtsError(RuntimeError):
    """A library call returned a negative DHTS_E_* status (`.status`; None for errors raised by the binding itself)."""
    status = None


def lib():
    """Load libdhts.so; raise loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise DhtsError(
                "libdhts.so not found at %s -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C diff-hybrid-traffic-sim_amd/csrc`). There is no CPU fallback." % SO_PATH)
        handle = C.CDLL(SO_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)       # AttributeError if the symbol is missing
            fn.restype = res
            fn.argtypes = args
            names = tuple(n for n, _ in PARAMETERS[name][1])
            _entries[name] = fn, names, (operator.itemgetter(*names) if len(names) > 1 else _few(names))
        _lib = handle
    return _lib


def _few(names):
    """operator.itemgetter for fewer than two names: it returns a tuple as well."""
    return (lambda given, n=names[0]: (given[n],)) if names else (lambda given: ())


def _ordered(name, args, kw):
    """-> (the entry's function, its arguments in the table's order) from the mapping `args`, or from the keywords `kw`, which must be
    exactly the parameters the entry declares; DhtsError otherwise."""
    try:
        fn, names, pick = _entries[name]
    except KeyError:
        lib()
        if name not in _entries:
            raise DhtsError("%s is not an entry point of include/dhts.h" % name) from None
        fn, names, pick = _entries[name]
    if args is not None and kw:
        raise TypeError("%s: a mapping or keywords, not both" % name)
    try:
        values = pick(kw if args is None else args)
    except KeyError as e:
        raise DhtsError("%s: parameter %s was not supplied" % (name, e)) from None
    if args is None and len(kw) != len(names):       # (every declared name was found: the others are the undeclared ones)
        raise DhtsError("%s declares no parameter %s" % (name, ", ".join(repr(k) for k in kw if k not in names)))
    return fn, values


def raw(name, args=None, **kw):
    """Call the entry point `name` with its arguments given by parameter name (include/dhts.h's names; the order is _TABLE's) and
    return what it returns.  Keywords: exactly the parameters the entry declares.  A mapping `args` instead: the entry takes the names
    it declares and ignores the rest (what a family of sibling entry points shares one mapping for).  A parameter that is not supplied,
    or a keyword the entry does not declare, is a DhtsError raised before the library is entered."""
    fn, values = _ordered(name, args, kw)
    return fn(*values)


def call(name, args=None, **kw):
    """raw() for an entry point that returns a DHTS_E_* status: a negative one raises DhtsError."""
    fn, values = _ordered(name, args, kw)
    status = fn(*values)
    if status != OK:
        check(status, name)


def bind(name):
    """call(name, ...) in the keyword form as a function of its own, the entry looked up once: for a loop that calls it per step."""
    lib()
    fn, names, pick = _entries[name]

    def bound(**kw):
        try:
            values = pick(kw)
        except KeyError as e:
            raise DhtsError("%s: parameter %s was not supplied" % (name, e)) from None
        if len(kw) != len(names):
            raise DhtsError("%s declares no parameter %s" % (name, ", ".join(repr(k) for k in kw if k not in names)))
        status = fn(*values)
        if status != OK:
            check(status, name)
    return bound


def check(status, what):
    if status != OK:
        names = {E_INVALID: "DHTS_E_INVALID (bad argument)", E_LAUNCH: "DHTS_E_LAUNCH (HIP launch failed)",
                 E_NO_DEVICE: "DHTS_E_NO_DEVICE"}
        e = DhtsError("%s failed: %s" % (what, names.get(status, status)))
        e.status = status
        raise e
