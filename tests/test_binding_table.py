"""The binding's one table of the C ABI (dhts._lib: _TABLE -> PARAMETERS -> SIGNATURES) against include/dhts.h, over every function
the header declares -- names, order, types, return types, exports -- and the by-name call path (_lib.raw / _lib.call) on two entry
points that need no device.  No GPU needed."""
import ctypes as C
import os
import re

import pytest

from dhts import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = {"dhts_macro_desc": _lib.MacroDesc, "dhts_micro_desc": _lib.MicroDesc, "dhts_net_desc": _lib.NetDesc,
           "dhts_net_tables": _lib.NetTables, "dhts_hybrid_tables": _lib.HybridTables, "dhts_hybrid_state_io": _lib.HybridStateIO,
           "dhts_netstep_tables": _lib.NetstepTables}
RETURNS = {"int": C.c_int, "size_t": C.c_size_t}


def header():
    """include/dhts.h -> {function: (return type, [(parameter name, C type with the array suffix, e.g. "int32_t[8]")])}, in its order."""
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dhts.h")).read(), flags=re.S)
    txt = re.sub(r"//[^\n]*", "", txt)
    out = {}
    for ret, name, params in re.findall(r"\b(\w+)\s+(dhts_\w+)\s*\(([^;{}()]*)\)\s*;", txt):
        assert name not in out, "%s is declared twice" % name
        out[name] = ret, []
        for a in ([] if params.strip() in ("", "void") else params.split(",")):
            m = re.fullmatch(r"(.*?)(\w+)\s*(\[\d+\])?", " ".join(a.split()))
            out[name][1].append((m.group(2), m.group(1).replace(" ", "") + (m.group(3) or "")))
    return out


def bound_type(function, name, ctype):
    """The one rule: what a parameter of C type `ctype` (spaces removed) binds to."""
    if ctype in ("int", "int32_t"):
        return C.c_int
    if ctype == "int64_t":
        return C.c_int64
    if ctype == "double":
        return C.c_double
    if ctype == "int32_t[8]":
        return C.POINTER(C.c_int32) if function == "dhts_net_hybrid_plan" else C.POINTER(C.c_int32 * 8)
    assert ctype.endswith("*"), "%s: %s %s is passed by value and the rule does not know it" % (function, ctype, name)
    pointee = ctype[:-1].replace("const", "")
    return C.POINTER(STRUCTS[pointee]) if pointee in STRUCTS else C.c_void_p


HEADER = header()


def test_the_header_parses_to_the_abi_it_is_known_to_declare():
    assert len(HEADER) == 103
    assert {ret for ret, _ in HEADER.values()} == set(RETURNS)
    for name, (_, params) in HEADER.items():
        names = [n for n, _ in params]
        assert len(set(names)) == len(names), "%s repeats a parameter name" % name
    used = {t[:-1].replace("const", "") for _, params in HEADER.values() for _, t in params if t.endswith("*")}
    assert set(STRUCTS) <= used, "a struct of the rule is passed nowhere"


def test_the_table_has_the_header_s_functions_and_no_other():
    assert set(_lib.PARAMETERS) == set(HEADER)
    assert set(_lib._TABLE) == set(HEADER)


@pytest.mark.parametrize("name", sorted(HEADER))
def test_every_function_is_bound_by_the_header_s_names_and_types(name):
    ret, params = HEADER[name]
    res, bound = _lib.PARAMETERS[name]
    assert res is RETURNS[ret]
    assert [n for n, _ in bound] == [n for n, _ in params]
    for (n, got), (_, ctype) in zip(bound, params):
        assert got is bound_type(name, n, ctype), (name, n, ctype, got)
    assert hasattr(_lib.lib(), name), "libdhts.so does not export %s" % name
    fn = getattr(_lib.lib(), name)
    assert fn.restype is res and list(fn.argtypes) == [t for _, t in bound]


def test_signatures_are_what_the_table_derives():
    assert _lib.SIGNATURES == {name: (res, [t for _, t in params]) for name, (res, params) in _lib.PARAMETERS.items()}
    assert list(_lib.SIGNATURES) == list(_lib.PARAMETERS)
    for res, args in _lib.SIGNATURES.values():
        assert isinstance(args, list)


# ---- the call path ------------------------------------------------------------------------------------------------------------------
def plan_args():
    d, plan = _lib.MacroDesc(3, 100, 0.01, 5.0, 30.0), (C.c_int32 * 8)()
    return d, plan, dict(d=C.byref(d), T=40, n_det=2, segment=0, plan=C.byref(plan))


def test_keywords_and_a_mapping_return_what_the_positional_call_returns():
    lib = _lib.lib()
    d, plan, args = plan_args()
    assert lib.dhts_macro_ckpt_plan(C.byref(d), 40, 2, 0, C.byref(plan)) == 0
    want = list(plan)
    assert want[2] >= 1
    for form in (lambda: _lib.raw("dhts_macro_ckpt_plan", **args), lambda: _lib.raw("dhts_macro_ckpt_plan", args),
                 lambda: _lib.call("dhts_macro_ckpt_plan", **args), lambda: _lib.call("dhts_macro_ckpt_plan", args)):
        C.memset(plan, 0, C.sizeof(plan))
        assert form() in (0, None) and list(plan) == want
    # the order of the keywords is not the order of the call
    C.memset(plan, 0, C.sizeof(plan))
    assert _lib.raw("dhts_macro_ckpt_plan", **dict(reversed(list(args.items())))) == 0 and list(plan) == want
    nbytes = lib.dhts_macro_ckpt_bytes(C.byref(d), 40, 7)
    assert nbytes > 0
    assert _lib.raw("dhts_macro_ckpt_bytes", d=C.byref(d), T=40, segment=7) == nbytes
    assert _lib.raw("dhts_macro_ckpt_bytes", dict(d=C.byref(d), T=40, segment=7)) == nbytes
    assert _lib.raw("dhts_macro_ckpt_bytes", d=C.byref(d), T=7, segment=40) == lib.dhts_macro_ckpt_bytes(C.byref(d), 7, 40) != nbytes


def test_a_mapping_may_hold_more_than_the_entry_declares():
    d, plan, args = plan_args()
    assert _lib.raw("dhts_macro_ckpt_plan", args) == 0
    want = list(plan)
    C.memset(plan, 0, C.sizeof(plan))
    assert _lib.raw("dhts_macro_ckpt_plan", dict(args, ring=1, ghost=None, n_ramp=5)) == 0 and list(plan) == want
    # the family's mapping serves the sibling that takes fewer of its names
    assert _lib.raw("dhts_macro_ckpt_bytes", args) == _lib.lib().dhts_macro_ckpt_bytes(C.byref(d), 40, 0)


@pytest.mark.parametrize("fn", [_lib.raw, _lib.call])
def test_a_missing_parameter_is_the_binding_s_error_before_the_library_is_entered(fn):
    d, plan, args = plan_args()
    for missing in args:
        some = {k: v for k, v in args.items() if k != missing}
        for form in (lambda: fn("dhts_macro_ckpt_plan", **some), lambda: fn("dhts_macro_ckpt_plan", some)):
            with pytest.raises(_lib.DhtsError, match=r"dhts_macro_ckpt_plan: parameter '%s' was not supplied" % missing) as e:
                form()
            assert e.value.status is None
    assert list(plan) == [0] * 8


@pytest.mark.parametrize("fn", [_lib.raw, _lib.call])
def test_an_undeclared_keyword_is_the_binding_s_error(fn):
    d, plan, args = plan_args()
    with pytest.raises(_lib.DhtsError, match=r"dhts_macro_ckpt_plan declares no parameter 'ring'") as e:
        fn("dhts_macro_ckpt_plan", ring=1, **args)
    assert e.value.status is None and list(plan) == [0] * 8
    with pytest.raises(TypeError, match="a mapping or keywords, not both"):
        fn("dhts_macro_ckpt_plan", args, segment=0)
    with pytest.raises(_lib.DhtsError, match="dhts_macro_ckpt_plans is not an entry point"):
        fn("dhts_macro_ckpt_plans", args)


def test_call_raises_on_a_negative_status_and_raw_returns_it():
    d, plan, args = plan_args()
    args["T"] = -1
    assert _lib.raw("dhts_macro_ckpt_plan", args) == _lib.E_INVALID
    with pytest.raises(_lib.DhtsError, match=r"dhts_macro_ckpt_plan failed: DHTS_E_INVALID \(bad argument\)") as e:
        _lib.call("dhts_macro_ckpt_plan", args)
    assert e.value.status == _lib.E_INVALID
    with pytest.raises(_lib.DhtsError, match="dhts_macro_ckpt_plan failed") as e:
        _lib.call("dhts_macro_ckpt_plan", **args)
    assert e.value.status == _lib.E_INVALID


def test_a_bound_entry_is_call_in_the_keyword_form():
    d, plan, args = plan_args()
    assert _lib.raw("dhts_macro_ckpt_plan", args) == 0
    want = list(plan)
    C.memset(plan, 0, C.sizeof(plan))
    ask = _lib.bind("dhts_macro_ckpt_plan")
    assert ask(**dict(reversed(list(args.items())))) is None and list(plan) == want
    with pytest.raises(_lib.DhtsError, match=r"dhts_macro_ckpt_plan: parameter 'segment' was not supplied"):
        ask(**{k: v for k, v in args.items() if k != "segment"})
    with pytest.raises(_lib.DhtsError, match=r"dhts_macro_ckpt_plan declares no parameter 'ring'"):
        ask(ring=1, **args)
    with pytest.raises(_lib.DhtsError, match="dhts_macro_ckpt_plan failed") as e:
        ask(**dict(args, T=-1))
    assert e.value.status == _lib.E_INVALID
