"""CPU: every ctypes mirror of _lib.py against include/dss2_hip.h as a C++ compiler reads it (tests/abi_probe.py): each struct's size and
each field's offset, size and kind; each entry point's return type, argument count and argument kinds, POINTER(S) to S's struct; each
integer constant; and that the three tables leave out nothing the header has.  Needs neither the built library nor a GPU.
The same probe is then handed deliberately broken copies of the tables and must name what is broken."""
import ctypes as C

import pytest

import abi_probe
from conftest import load_pkg


@pytest.fixture(scope="module")
def L():
    return load_pkg()._lib


def constants(L):
    return {k: v for k, v in vars(L).items() if k.isupper() and isinstance(v, int)}


def mirror(cls, fields):
    return type(cls.__name__, (C.Structure,), {"_fields_": fields})


def test_mirrors_signatures_and_constants_match_the_header(L):
    bad = abi_probe.mismatches(L.C_STRUCTS, L._SIGNATURES, constants(L))
    print(f"[abi] {len(L.C_STRUCTS)} structs, {sum(len(c._fields_) for c in L.C_STRUCTS.values())} fields, "
          f"{len(L._SIGNATURES)} functions, {len(constants(L))} constants")
    assert not bad, "\n".join(bad)


def test_the_tables_leave_out_nothing_the_header_has(L):
    assert abi_probe.header_struct_tags() == set(L.C_STRUCTS) and len(set(L.C_STRUCTS.values())) == len(L.C_STRUCTS)
    assert abi_probe.header_constants() == set(constants(L))
    # a field carries the C member's name; a trailing underscore where that is a Python keyword, or where C has it too (pad_)
    assert {f for cls in L.C_STRUCTS.values() for f, _ in cls._fields_ if f.endswith("_")} == {"lambda_", "pad_"}


def test_two_swapped_fields_of_equal_size_are_reported(L):
    f = list(L.GemmPropArgs._fields_)
    i, j = f.index(("Bp", C.c_void_p)), f.index(("bias", C.c_void_p))
    f[i], f[j] = f[j], f[i]
    bad = abi_probe.mismatches({"dss2_gemm_prop_args": mirror(L.GemmPropArgs, f)}, {}, {})
    assert len(bad) == 2 and "dss2_gemm_prop_args field bias: header offset 32" in bad[0] and "dss2_gemm_prop_args field Bp: header offset 24" in bad[1], bad


def test_a_field_of_the_wrong_type_and_the_right_size_is_reported(L):
    f = [(n, C.c_int32 if n == "drop_scale" else t) for n, t in L.GemmPropArgs._fields_]
    bad = abi_probe.mismatches({"dss2_gemm_prop_args": mirror(L.GemmPropArgs, f)}, {}, {})
    assert len(bad) == 1 and "dss2_gemm_prop_args field drop_scale:" in bad[0] and "kind f4" in bad[0] and "kind i4" in bad[0], bad


def test_a_narrowed_argument_is_reported(L):
    res, args = L._SIGNATURES["dss2_eval_batch"]
    i = args.index(C.c_int64)
    sigs = dict(L._SIGNATURES, dss2_eval_batch=(res, args[:i] + [C.c_int] + args[i + 1:]))
    assert abi_probe.mismatches(L.C_STRUCTS, sigs, {}) == [f"function dss2_eval_batch argument {i}: header i8, mirror i4"]


def test_a_pointer_to_the_wrong_struct_is_reported(L):
    sigs = dict(L._SIGNATURES, dss2_wls_solve_large=(C.c_int, [C.POINTER(L.WlsSolveArgs), C.c_void_p]))
    assert abi_probe.mismatches(L.C_STRUCTS, sigs, {}) == \
        ["function dss2_wls_solve_large argument 0: header p>s:dss2_wls_large_args, mirror p>s:dss2_wls_solve_args"]


def test_a_missing_registry_entry_is_reported(L):
    assert abi_probe.header_struct_tags() - (set(L.C_STRUCTS) - {"dss2_reduce_desc"}) == {"dss2_reduce_desc"}
    # ... and a struct that a nested field or a POINTER names without being registered has no tag on either side
    short = {k: v for k, v in L.C_STRUCTS.items() if k != "dss2_wls_solve_args"}
    bad = abi_probe.mismatches(short, {"dss2_wls_large_groups": L._SIGNATURES["dss2_wls_large_groups"]}, {})
    assert any("dss2_wls_large_args field solve:" in b and "?WlsSolveArgs" in b for b in bad), bad
    assert "function dss2_wls_large_groups argument 0: header p>?, mirror p>s:?WlsSolveArgs" in bad


def test_a_constant_off_by_one_is_reported(L):
    bad = abi_probe.mismatches({}, {}, dict(constants(L), WGRAD_F16_TALL=L.WGRAD_F16_TALL + 1))
    assert bad == [f"constant WGRAD_F16_TALL: header DSS2_WGRAD_F16_TALL = {L.WGRAD_F16_TALL}, mirror {L.WGRAD_F16_TALL + 1}"]


def test_a_name_the_header_does_not_have_is_reported(L):
    bad = abi_probe.mismatches({"dss2_no_such_args": L.GradDesc}, {"dss2_no_such_entry": (C.c_int, [])}, {"NO_SUCH": 1})
    assert bad == [f"{what}: not declared in include/dss2_hip.h" for what in ("struct dss2_no_such_args", "function dss2_no_such_entry", "constant DSS2_NO_SUCH")]
    bad = abi_probe.mismatches({"dss2_grad_desc": mirror(L.GradDesc, [("grad", C.c_void_p), ("count", C.c_int64)])}, {}, {})
    assert len(bad) == 1 and "does not compile" in bad[0] and "count" in bad[0], bad
