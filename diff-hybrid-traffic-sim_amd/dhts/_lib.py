"""ctypes binding of libdhts.so (C ABI: include/dhts.h).

The shared object is built in-tree by `diff-hybrid-traffic-sim_amd/csrc/Makefile` (driven by
`__graft_entry__.build()`).  There is NO fallback: if the library is missing or a call fails, an exception
is raised -- the product path never routes through a CPU implementation.
"""
import ctypes as C
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


# name -> (restype, argtypes); every symbol include/dhts.h declares
_P = C.c_void_p
SIGNATURES = {
    "dhts_version": (C.c_int, []),
    "dhts_device_count": (C.c_int, []),
    "dhts_set_option": (C.c_int, [C.c_int, C.c_int]),
    "dhts_padded": (C.c_int, [C.c_int]),
    "dhts_macro_tape_bytes": (C.c_size_t, [C.POINTER(MacroDesc), C.c_int]),
    "dhts_macro_step_tape_bytes": (C.c_size_t, [C.POINTER(MacroDesc)]),
    "dhts_arz_interface_batch": (C.c_int, [C.c_int64, C.c_int, _P, C.c_double, C.c_double] + [_P] * 11),
    "dhts_idm_batch": (C.c_int, [C.c_int64, C.c_int] + [_P] * 8),
    "dhts_idm_jac_batch": (C.c_int, [C.c_int64] + [_P] * 4),
    "dhts_macro_state_from_ru": (C.c_int, [C.c_int64, C.c_double, _P, _P, _P, _P, _P]),
    "dhts_macro_state_from_ru_bwd": (C.c_int, [C.c_int64, C.c_double, _P, _P, _P, _P, _P, _P]),
    "dhts_macro_u_tap_bwd": (C.c_int, [C.c_int64, C.c_double, _P, _P, _P, _P, _P, _P]),
    "dhts_macro_rollout_fwd": (C.c_int, [C.POINTER(MacroDesc), C.c_int] + [_P] * 13),
    "dhts_macro_rollout_bwd": (C.c_int, [C.POINTER(MacroDesc), C.c_int] + [_P] * 9),
    "dhts_macro_rollout_fwd_sched": (C.c_int, [C.POINTER(MacroDesc), C.c_int] + [_P] * 13),
    "dhts_macro_rollout_bwd_sched": (C.c_int, [C.POINTER(MacroDesc), C.c_int] + [_P] * 9),
    "dhts_macro_rollout_plan": (C.c_int, [C.POINTER(MacroDesc), C.c_int, C.c_int, C.POINTER(C.c_int32 * 8)]),
    "dhts_macro_rollout_fwd_taps": (C.c_int, [C.POINTER(MacroDesc), C.c_int] + [_P] * 5 + [C.c_int] + [_P] * 6 + [C.c_int] + [_P] * 3),
    "dhts_macro_rollout_bwd_taps": (C.c_int, [C.POINTER(MacroDesc), C.c_int] + [_P] * 4 + [C.c_int] + [_P] * 4 + [C.c_int] + [_P] * 2),
    "dhts_macro_taps_plan": (C.c_int, [C.POINTER(MacroDesc), C.c_int, C.c_int, C.POINTER(C.c_int32 * 8)]),
    "dhts_macro_rollout_jvp": (C.c_int, [C.POINTER(MacroDesc), C.c_int, _P, C.c_int] + [_P] * 3 + [C.c_int] + [_P] * 3 + [C.c_int] + [_P] * 3),
    "dhts_macro_jvp_plan": (C.c_int, [C.POINTER(MacroDesc), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32 * 8)]),
    "dhts_macro_rollout_fwd_jvp": (C.c_int, [C.POINTER(MacroDesc), C.c_int, C.c_int] + [_P] * 5 + [C.c_int] + [_P] * 10 + [C.c_int] + [_P] * 5),
    "dhts_macro_fwd_jvp_plan": (C.c_int, [C.POINTER(MacroDesc), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32 * 8)]),
    "dhts_macro_ckpt_plan": (C.c_int, [C.POINTER(MacroDesc), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32 * 8)]),
    "dhts_macro_ckpt_bytes": (C.c_size_t, [C.POINTER(MacroDesc), C.c_int, C.c_int]),
    "dhts_macro_rollout_fwd_ckpt": (C.c_int, [C.POINTER(MacroDesc), C.c_int, C.c_int] + [_P] * 5 + [C.c_int] + [_P] * 5 + [C.c_int] + [_P] * 4),
    "dhts_macro_rollout_bwd_ckpt": (C.c_int, [C.POINTER(MacroDesc), C.c_int, C.c_int] + [_P] * 6 + [C.c_int] + [_P] * 3 + [C.c_int] + [_P] * 6),
    "dhts_macro_ckpt_target_plan": (C.c_int, [C.POINTER(MacroDesc), C.c_int, C.c_int, C.POINTER(C.c_int32 * 8)]),
    "dhts_macro_rollout_fwd_ckpt_target": (C.c_int, [C.POINTER(MacroDesc), C.c_int, C.c_int] + [_P] * 5 + [C.c_int] + [_P] * 9),
    "dhts_macro_rollout_bwd_ckpt_target": (C.c_int, [C.POINTER(MacroDesc), C.c_int, C.c_int] + [_P] * 6 + [C.c_int] + [_P] * 12),
    "dhts_macro_state_from_ru_jvp": (C.c_int, [C.c_int64, C.c_double] + [_P] * 6),
    "dhts_macro_u_tap_jvp": (C.c_int, [C.c_int64, C.c_double] + [_P] * 6),
    "dhts_macro_tape_expand": (C.c_int, [C.POINTER(MacroDesc), C.c_int] + [_P] * 3),
    "dhts_macro_step_fwd": (C.c_int, [C.POINTER(MacroDesc)] + [_P] * 12),
    "dhts_macro_step_bwd": (C.c_int, [C.POINTER(MacroDesc)] + [_P] * 8),
    "dhts_net_macro_hist_bytes": (C.c_size_t, [C.POINTER(NetDesc)]),
    "dhts_net_macro_tape_bytes": (C.c_size_t, [C.POINTER(NetDesc)]),
    "dhts_net_macro_plan": (C.c_int, [C.POINTER(NetDesc), C.POINTER(C.c_int32 * 8)]),
    "dhts_net_macro_rollout_fwd": (C.c_int, [C.POINTER(NetDesc), C.POINTER(NetTables)] + [_P] * 9),
    "dhts_net_macro_rollout_eval": (C.c_int, [C.POINTER(NetDesc), C.POINTER(NetTables)] + [_P] * 5),
    "dhts_net_macro_rollout_bwd": (C.c_int, [C.POINTER(NetDesc), C.POINTER(NetTables)] + [_P] * 10),
    "dhts_net_ghosts_fwd": (C.c_int, [C.POINTER(NetDesc), C.POINTER(NetTables), C.c_int, C.c_int] + [_P] * 7),
    "dhts_net_ghosts_bwd": (C.c_int, [C.POINTER(NetDesc), C.POINTER(NetTables), _P, _P, C.c_int] + [_P] * 13),
    "dhts_net_hybrid_tape_bytes": (C.c_size_t, [C.POINTER(NetDesc)]),
    "dhts_net_hybrid_workspace_bytes": (C.c_size_t, [C.POINTER(NetDesc), C.POINTER(HybridTables)]),
    "dhts_net_hybrid_plan": (C.c_int, [C.POINTER(NetDesc), C.POINTER(HybridTables), C.POINTER(C.c_int32)]),
    "dhts_net_hybrid_rollout_fwd": (C.c_int, [C.POINTER(NetDesc), C.POINTER(HybridTables)] + [_P] * 10),
    "dhts_net_hybrid_rollout_eval": (C.c_int, [C.POINTER(NetDesc), C.POINTER(HybridTables)] + [_P] * 6),
    "dhts_net_hybrid_rollout_bwd": (C.c_int, [C.POINTER(NetDesc), C.POINTER(HybridTables)] + [_P] * 10),
    "dhts_net_hybrid_state_rollout_fwd": (C.c_int, [C.POINTER(NetDesc), C.POINTER(HybridTables), C.POINTER(HybridStateIO)] + [_P] * 10),
    "dhts_net_hybrid_state_rollout_bwd": (C.c_int, [C.POINTER(NetDesc), C.POINTER(HybridTables), C.c_int32] + [_P] * 13),
    "dhts_netstep_workspace_bytes": (C.c_size_t, [C.POINTER(NetDesc), C.POINTER(NetstepTables)]),
    "dhts_netstep_rollout_fwd": (C.c_int, [C.POINTER(NetDesc), C.POINTER(NetstepTables), C.c_int] + [_P] * 8),
    "dhts_netstep_rollout_bwd": (C.c_int, [C.POINTER(NetDesc), C.POINTER(NetstepTables)] + [_P] * 8),
    "dhts_micro_tape_bytes": (C.c_size_t, [C.POINTER(MicroDesc), C.c_int]),
    "dhts_micro_step_tape_bytes": (C.c_size_t, [C.POINTER(MicroDesc)]),
    "dhts_micro_rollout_fwd": (C.c_int, [C.POINTER(MicroDesc), C.c_int] + [_P] * 11),
    "dhts_micro_rollout_bwd": (C.c_int, [C.POINTER(MicroDesc), C.c_int] + [_P] * 10),
    "dhts_micro_param_tape_bytes": (C.c_size_t, [C.POINTER(MicroDesc), C.c_int]),
    "dhts_micro_rollout_fwd_params": (C.c_int, [C.POINTER(MicroDesc), C.c_int] + [_P] * 12),
    "dhts_micro_rollout_bwd_params": (C.c_int, [C.POINTER(MicroDesc), C.c_int] + [_P] * 13),
    "dhts_idm_param_jac_batch": (C.c_int, [C.c_int64] + [_P] * 4),
    "dhts_micro_rollout_plan": (C.c_int, [C.POINTER(MicroDesc), C.c_int, C.c_int, C.POINTER(C.c_int32 * 8)]),
    "dhts_micro_rollout_jvp": (C.c_int, [C.POINTER(MicroDesc), C.c_int, C.c_int] + [_P] * 13),
    "dhts_micro_jvp_plan": (C.c_int, [C.POINTER(MicroDesc), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32 * 8)]),
    "dhts_micro_rollout_fwd_jvp": (C.c_int, [C.POINTER(MicroDesc), C.c_int, C.c_int] + [_P] * 18),
    "dhts_micro_fwd_jvp_plan": (C.c_int, [C.POINTER(MicroDesc), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32 * 8)]),
    "dhts_micro_ckpt_plan": (C.c_int, [C.POINTER(MicroDesc), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32 * 8)]),
    "dhts_micro_ckpt_bytes": (C.c_size_t, [C.POINTER(MicroDesc), C.c_int, C.c_int]),
    "dhts_micro_rollout_fwd_ckpt": (C.c_int, [C.POINTER(MicroDesc), C.c_int, C.c_int] + [_P] * 11),
    "dhts_micro_rollout_bwd_ckpt": (C.c_int, [C.POINTER(MicroDesc), C.c_int, C.c_int] + [_P] * 13),
    "dhts_micro_rollout_fwd_ckpt_samples": (C.c_int, [C.POINTER(MicroDesc), C.c_int, C.c_int] + [_P] * 9 + [C.c_int, C.c_int] + [_P] * 3),
    "dhts_micro_rollout_bwd_ckpt_samples": (C.c_int, [C.POINTER(MicroDesc), C.c_int, C.c_int] + [_P] * 7 + [C.c_int, C.c_int] + [_P] * 7),
    "dhts_micro_rollout_fwd_jvp_samples": (C.c_int, [C.POINTER(MicroDesc), C.c_int, C.c_int] + [_P] * 14 + [C.c_int, C.c_int] + [_P] * 5),
    "dhts_micro_rollout_fwd_ckpt_lead": (C.c_int, [C.POINTER(MicroDesc), C.c_int, C.c_int] + [_P] * 10 + [C.c_int, C.c_int] + [_P] * 3),
    "dhts_micro_rollout_bwd_ckpt_lead": (C.c_int, [C.POINTER(MicroDesc), C.c_int, C.c_int] + [_P] * 8 + [C.c_int, C.c_int] + [_P] * 7),
    "dhts_micro_rollout_fwd_jvp_lead": (C.c_int, [C.POINTER(MicroDesc), C.c_int, C.c_int] + [_P] * 15 + [C.c_int, C.c_int] + [_P] * 5),
    "dhts_micro_ckpt_target_plan": (C.c_int, [C.POINTER(MicroDesc), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32 * 8)]),
    "dhts_micro_rollout_fwd_ckpt_target": (C.c_int, [C.POINTER(MicroDesc), C.c_int, C.c_int] + [_P] * 14),
    "dhts_micro_rollout_bwd_ckpt_target": (C.c_int, [C.POINTER(MicroDesc), C.c_int, C.c_int] + [_P] * 17),
    "dhts_macro_rollout_fwd_ckpt_ring": (C.c_int, [C.POINTER(MacroDesc), C.c_int, C.c_int] + [_P] * 9 + [C.c_int] + [_P] * 4),
    "dhts_macro_rollout_bwd_ckpt_ring": (C.c_int, [C.POINTER(MacroDesc), C.c_int, C.c_int] + [_P] * 8 + [C.c_int] + [_P] * 5),
    "dhts_macro_rollout_fwd_ckpt_target_ring": (C.c_int, [C.POINTER(MacroDesc), C.c_int, C.c_int] + [_P] * 13),
    "dhts_macro_rollout_bwd_ckpt_target_ring": (C.c_int, [C.POINTER(MacroDesc), C.c_int, C.c_int] + [_P] * 16),
    "dhts_macro_rollout_fwd_jvp_ring": (C.c_int, [C.POINTER(MacroDesc), C.c_int, C.c_int] + [_P] * 13 + [C.c_int] + [_P] * 5),
    "dhts_micro_rollout_fwd_ckpt_ring": (C.c_int, [C.POINTER(MicroDesc), C.c_int, C.c_int] + [_P] * 9 + [C.c_int, C.c_int] + [_P] * 3),
    "dhts_micro_rollout_bwd_ckpt_ring": (C.c_int, [C.POINTER(MicroDesc), C.c_int, C.c_int] + [_P] * 7 + [C.c_int, C.c_int] + [_P] * 6),
    "dhts_micro_rollout_fwd_jvp_ring": (C.c_int, [C.POINTER(MicroDesc), C.c_int, C.c_int] + [_P] * 13 + [C.c_int, C.c_int] + [_P] * 5),
    # desc T n_dir | p v count params | head lead lead_length ring | t_p t_v t_head t_lead t_params | the four outputs | probes n_probes
    # every | target sse jtr jtj | err err_jvp stream
    "dhts_micro_rollout_fwd_jvp_gn": (C.c_int, [C.POINTER(MicroDesc), C.c_int, C.c_int] + [_P] * 18 + [C.c_int, C.c_int] + [_P] * 7),
    "dhts_micro_fwd_jvp_gn_plan": (C.c_int, [C.POINTER(MicroDesc), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32 * 8)]),
    "dhts_micro_rollout_fwd_ckpt_target_ring": (C.c_int, [C.POINTER(MicroDesc), C.c_int, C.c_int] + [_P] * 12),
    "dhts_micro_rollout_bwd_ckpt_target_ring": (C.c_int, [C.POINTER(MicroDesc), C.c_int, C.c_int] + [_P] * 13),
    # the siblings' arguments, then ramps, n_ramp, inflow (reverse: and g_inflow), ring, err, stream
    "dhts_macro_rollout_fwd_ckpt_ramp": (C.c_int, [C.POINTER(MacroDesc), C.c_int, C.c_int] + [_P] * 5 + [C.c_int] + [_P] * 5 + [C.c_int] +
                                         [_P] * 3 + [C.c_int, _P, C.c_int] + [_P] * 2),
    "dhts_macro_rollout_bwd_ckpt_ramp": (C.c_int, [C.POINTER(MacroDesc), C.c_int, C.c_int] + [_P] * 6 + [C.c_int] + [_P] * 3 + [C.c_int] +
                                         [_P] * 5 + [C.c_int, _P, _P, C.c_int] + [_P] * 2),
    "dhts_macro_rollout_fwd_ckpt_target_ramp": (C.c_int, [C.POINTER(MacroDesc), C.c_int, C.c_int] + [_P] * 5 + [C.c_int] + [_P] * 8 +
                                                [C.c_int, _P, C.c_int] + [_P] * 2),
    "dhts_macro_rollout_bwd_ckpt_target_ramp": (C.c_int, [C.POINTER(MacroDesc), C.c_int, C.c_int] + [_P] * 6 + [C.c_int] + [_P] * 11 +
                                                [C.c_int, _P, _P, C.c_int] + [_P] * 2),
    # the siblings' arguments, then ramps, n_ramp, inflow, t_inflow
    "dhts_macro_rollout_fwd_jvp_ramp": (C.c_int, [C.POINTER(MacroDesc), C.c_int, C.c_int] + [_P] * 5 + [C.c_int] + [_P] * 10 + [C.c_int] +
                                        [_P] * 5 + [_P, C.c_int, _P, _P]),
    "dhts_macro_rollout_fwd_jvp_ring_ramp": (C.c_int, [C.POINTER(MacroDesc), C.c_int, C.c_int] + [_P] * 13 + [C.c_int] + [_P] * 5 +
                                             [_P, C.c_int, _P, _P]),
    "dhts_micro_step_fwd": (C.c_int, [C.POINTER(MicroDesc)] + [_P] * 10),
    "dhts_micro_step_fwd_tensor": (C.c_int, [C.POINTER(MicroDesc)] + [_P] * 10),
    "dhts_micro_step_fwd_tensor_head": (C.c_int, [C.POINTER(MicroDesc)] + [_P] * 10),
    "dhts_micro_step_bwd": (C.c_int, [C.POINTER(MicroDesc)] + [_P] * 9),
}

_lib = None


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
        _lib = handle
    return _lib


def check(status, what):
    if status != OK:
        names = {E_INVALID: "DHTS_E_INVALID (bad argument)", E_LAUNCH: "DHTS_E_LAUNCH (HIP launch failed)",
                 E_NO_DEVICE: "DHTS_E_NO_DEVICE"}
        e = DhtsError("%s failed: %s" % (what, names.get(status, status)))
        e.status = status
        raise e
