"""Closure of the leading-dimension table (tests/layout_cases.py) over include/f16_hip.h, without a GPU: every entry point the
contract applies to has a row or a named padded test elsewhere; a row lists exactly the array parameters the header declares; and
the comparison the GPU module relies on reports a kernel that indexes with B, writes a column too many or clears a foreign bit --
shown here on numpy stand-ins."""
import os
import re

import numpy as np
import pytest

import layout_cases as lc
from conftest import REPO


def functions():
    from f16_mpc_oop_py_amd import cabi, lib      # noqa: F401  (lib binds the header's structs to their ctypes classes)
    return cabi.functions()


def uncovered(fns):
    return [s for s in lc.contract_symbols(fns) if s not in lc.ROWS and s not in lc.COVERED_ELSEWHERE]


def test_every_entry_point_with_a_leading_dimension_has_a_row_or_a_named_test():
    fns = functions()
    syms = lc.contract_symbols(fns)
    assert "f16_rollout" in syms and "f16_mpc_plan_solve" in syms and "f16_rollout_mpc" in syms and len(syms) >= 52
    assert "f16_mpc_plan_warm_start" not in syms and "f16_mpc_plan_soft_rows" not in syms and "f16_debug_sincos" not in syms
    assert not [s for s in syms if s.startswith("f16_debug_elem_") or s == "f16_debug_air_triple"]   # host-pointer test entries: no leading dimension
    assert not uncovered(fns), f"no row in tests/layout_cases.py and no padded test named for: {uncovered(fns)}"
    assert not set(lc.ROWS) & set(lc.COVERED_ELSEWHERE)
    stray = [s for s in list(lc.ROWS) + list(lc.COVERED_ELSEWHERE) if s not in syms]
    assert not stray, f"not an entry point with a leading dimension: {stray}"
    assert {s for c in lc.CASES for s in c.symbols} == set(lc.ROWS), "a row without a case (or a case without a row)"
    assert len({c.id for c in lc.CASES}) == len(lc.CASES)


def test_a_new_entry_point_or_a_removed_row_is_named():
    from f16_mpc_oop_py_amd import cabi
    text = open(cabi.HEADER).read().replace("int f16_create(", "int f16_x(f16_ctx *ctx, double *p, long B, long ld);\nint f16_create(")
    assert uncovered(cabi.parse(text)[0]) == ["f16_x"]
    row = lc.ROWS.pop("f16_c2d_batch")
    try:
        assert uncovered(functions()) == ["f16_c2d_batch"]
    finally:
        lc.ROWS["f16_c2d_batch"] = row


@pytest.mark.parametrize("symbol", sorted(lc.COVERED_ELSEWHERE))
def test_the_named_test_exists_and_names_the_symbol(symbol):
    """read as text, not imported: the file exists, defines that test, and contains the symbol's name"""
    path, test = lc.COVERED_ELSEWHERE[symbol]
    text = open(os.path.join(REPO, path)).read()
    assert re.search(r"^def %s\(" % re.escape(test), text, flags=re.M), (path, test)
    assert re.search(r"\b%s\b" % re.escape(symbol), text), (path, symbol)


@pytest.mark.parametrize("symbol", sorted(lc.ROWS))
def test_a_row_lists_the_array_parameters_of_the_header(symbol):
    params = functions()[symbol][1]
    listed = [a.name for a in lc.ROWS[symbol].args]
    assert len(set(listed)) == len(listed)
    assert sorted(listed) == sorted(lc.array_parameters(params)), symbol
    names = [p for _, p in params]
    for a in lc.ROWS[symbol].args:
        assert a.ld is None or a.ld in names or "plan" in names, (symbol, a.name, a.ld)      # (a plan call: the ld of its creation)
        assert (a.dtype == "i4") == (a.name in ("status", "iters_traj", "gs_out")), (symbol, a.name)


def test_the_constants_of_the_cases_are_the_header_s():
    from f16_mpc_oop_py_amd import cabi
    c = cabi.constants()
    assert (lc.EULER, lc.RK4, lc.ONE_LANE) == (c["F16_INT_EULER"], c["F16_INT_RK4"], c["F16_FLAG_ONE_LANE"])
    assert not any(lc.FOREIGN & v for k, v in c.items() if k.startswith("F16_ST_")) and lc.FOREIGN != 1 << 8 + 18      # (no bit a kernel sets)
    assert [lc.padded_ld(B) for B in (1, 2, 19, 20, 65, 131100)] == [5, 5, 23, 23, 69, 131103]
    assert lc.OFFSET >= lc.GUARD and lc.OFFSET * 8 % 16 == 8 and lc.OFFSET * 4 % 16 == 4
    assert np.isnan(np.array(lc.SENT_F64, dtype=np.int64).view(np.float64)) and lc.SENT_F64 != lc.NAN_F64


# ------------------------------------------------------------------------------------------------ the harness on numpy stand-ins
TOY = lc.Row(lc.I("a", 3), lc.IO("x", 2), lc.O("y", 3), lc.O("extra", 1, optional=True), lc.ST(), status="sticky")
TOY_COST = lc.Row(lc.I("a", 3), lc.O("y", 3), lc.Arg("status", 1, "out", dtype="i4", optional=True), status="output")


def toy_kernel(bufs, B, ld, bug=None):
    """y[k][b] = 2 a[k][b]; x[k][b] += 1; extra[b] = a[0][b]; status[b] |= 1 -- on the flat arrays, indexed as a device kernel would"""
    def flat(name):
        b = bufs[name]
        if b.null:
            return None, 0
        b.after = b.full.copy()
        return (b.after.view(np.float64) if b.f8 else b.after), b.off
    (a, oa), (x, ox), (y, oy), (e, oe), (st, os_) = (flat(k) if k in bufs else (None, 0) for k in ("a", "x", "y", "extra", "status"))
    stride = B if bug == "index_B" else ld
    for b in range(B + (1 if bug == "one_column_too_many" else 0)):
        for k in range(3):
            y[oy + k * stride + b] = 2.0 * a[oa + k * ld + b]
        for k in range(2 if x is not None else 0):
            x[ox + k * ld + b] += 1.0
        if e is not None:
            e[oe + b] = a[oa + b]
        if st is not None:
            st[os_ + b] = 1 if bug == "clears_foreign" or "x" not in bufs else st[os_ + b] | 1
    if bug == "guard":
        y[oy - 1] = 0.0
    if bug == "reads_padding":
        y[oy] = a[oa + B] + 1.0


def toy(row, bug=None, B=5, null=False):
    data = dict(a=np.arange(3 * B, dtype=np.float64).reshape(3, B) + 0.5, x=-np.arange(2 * B, dtype=np.float64).reshape(2, B))
    tight, ld, _ = lc.layout(row.args, {}, B, B, False, data, row.status)
    toy_kernel(tight, B, ld)
    padded, ld, _ = lc.layout(row.args, {}, B, B, True, data, row.status, null)
    toy_kernel(padded, B, ld, bug)
    return tight, padded


def test_the_comparison_passes_a_correct_kernel():
    for row in (TOY, TOY_COST):
        tight, padded = toy(row)
        assert lc.compare(row.args, row.status, tight, padded) == []
        assert padded["y"].ld == 9 and padded["y"].off == lc.OFFSET and len(padded["y"].full) == lc.OFFSET + 27 + lc.GUARD
        _, bare = toy(row, null=True)
        assert bare["status"].null and lc.compare_required(row.args, padded, bare) == []
    tight, padded = toy(TOY)
    assert (tight["status"].after == 1).all() and (padded["status"].view(padded["status"].after)[0, :5] == lc.FOREIGN | 1).all()


@pytest.mark.parametrize("bug,words", [("index_B", ["y: columns < B differ", "y: padding columns"]), ("one_column_too_many", ["y: padding columns", "extra: padding columns"]),
                                       ("clears_foreign", ["status: a foreign bit"]), ("guard", ["y: a guard element before"]),
                                       ("reads_padding", ["y: columns < B differ"])])
def test_the_comparison_reports_a_wrong_kernel(bug, words):
    tight, padded = toy(TOY, bug)
    found = lc.compare(TOY.args, TOY.status, tight, padded)
    for w in words:
        assert any(w in f for f in found), (bug, w, found)


def test_an_output_status_is_compared_whole_and_a_missing_optional_output_must_not_change_the_rest():
    tight, padded = toy(TOY_COST)
    padded["status"].view(padded["status"].after)[0, 2] |= 8
    assert any("status: columns < B differ" in f for f in lc.compare(TOY_COST.args, TOY_COST.status, tight, padded))
    tight, padded = toy(TOY)
    _, bare = toy(TOY, null=True)
    bare["y"].view(bare["y"].after)[1, 1] ^= 1
    assert any(f.startswith("y: differs") for f in lc.compare_required(TOY.args, padded, bare))
