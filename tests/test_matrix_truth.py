"""The plain reference of the matrix probe, held to the oracle's CPU matrices before any GPU run (no GPU needed).

`oracle/groundtruth.c` states cells, row verdicts, rightmost active columns, walks and match words on integers and characters.
Here its verdicts, first columns and every cell of at most maxED are compared with `oracle_driver`'s `matrix` (64-bit) and
`matrix128` / `matrix128i` (128-bit) on every generated case — those matrices are pinned to the reference's bitparallelmatrix.cpp by
tests/golden/ref_vectors.out.  A row's verdict is the outcome of the whole chain of rightmost active columns before it, so this is
what proves the integer reading of bitparallelmatrix.h:398-412.  Then the comparators themselves: each must reject one changed
cell, verdict, RAC, CIGAR run or word bit, and accept a changed cell that stays above maxED.  Last, the probe must compile with
the library's flags.
"""
import numpy as np
import pytest

import matrixtruth as mt

GEO_NAMES = [g["name"] for g in mt.GEOS]


@pytest.mark.parametrize("name", GEO_NAMES)
def test_plain_reference_equals_pinned_matrices(oracle_built, name):
    cases, exps, counts, screened = mt.matrix_cases(name)
    oracle = mt.oracle_rows(name)
    n_rows = n_cells = n_exact = 0
    for ci, (case, exp, orows) in enumerate(zip(cases, exps, oracle)):
        k = case["k"]
        assert len(orows) == exp["rows"], (name, ci, case, "rows")
        for r, (v, fc, _, cells) in enumerate(orows):
            assert v == exp["v"][r], (name, ci, r + 1, case, "verdict")
            assert fc == exp["fc"][r] and len(cells) == exp["nc"][r], (name, ci, r + 1, case, "first column")
            e = exp["cells"][r, :len(cells)].astype(np.int64)
            wrong = np.where(e <= k, cells != e, cells <= k)
            assert not wrong.any(), (name, ci, r + 1, case, e.tolist(), cells.tolist())
            n_cells += len(e)
            n_exact += int((e <= k).sum())
        n_rows += len(orows)
    print(f"{name}: {len(cases)} cases, {n_rows} rows, {n_cells} cells ({n_exact} at most maxED) equal to the pinned CPU matrix")


@pytest.mark.parametrize("name", GEO_NAMES)
def test_matrix_case_set_meets_its_quotas(name):
    cases, exps, counts, screened = mt.matrix_cases(name)
    print(f"{name}: {len(cases)} cases, {screened} candidates screened; {mt.format_counts(counts)}")
    for q, need in mt.QUOTAS.items():
        assert sum(counts[q].values()) >= need, (name, q, counts[q], "quota not met within the screening cap")
    geo = mt.GEO[name]
    lengths = {len(c["x"]) for c in cases}
    assert set(mt.MAIN_LENGTHS + mt.LONG_LENGTHS) <= lengths
    assert {c["k"] for c in cases} == set(geo["ks"])
    if geo["intext"]:
        assert {(c["k"], c["nzeros"]) for c in cases} >= {(k, z) for k in geo["ks"] for z in (1, 2 * k + 1)}
        assert {(c["k"], c["off"]) for c in cases if c["nzeros"] == 2 * c["k"] + 1} >= {(k, off) for k in geo["ks"] for off in range(2 * k + 1)}
    else:
        assert max(len(c["init"]) for c in cases) > 4 and any(c["increase"] for c in cases)
    assert any(b"N" in c["x"] for c in cases)


@pytest.mark.parametrize("narrow", [True, False], ids=["narrow", "wide"])
def test_trace_case_set_meets_its_quotas(narrow):
    cases, exps, counts, screened = mt.trace_cases(narrow)
    print(f"{'narrow' if narrow else 'wide'} rows: {len(cases)} cases, {sum(e['n'] for e in exps)} walks, {screened} candidates screened; "
          f"{mt.format_counts(counts)}")
    for q, need in mt.TRACE_QUOTAS.items():
        assert sum(counts[q].values()) >= need, (narrow, q, counts[q], "quota not met within the screening cap")
    assert {c["k"] for c in cases} == set(range(1, 5 if narrow else 8))
    assert {(c["k"], c["off"]) for c in cases if c["nzeros"] > 1} >= {(k, off) for k in range(1, 5 if narrow else 8) for off in range(2 * k + 1)}


def _a_case(name, want):
    """the first case of a geometry with a valid row that has a cell of at most maxED and one above it"""
    cases, exps, _, _ = mt.matrix_cases(name)
    for case, exp in zip(cases, exps):
        if want(case, exp):
            return case, exp
    raise AssertionError("no such case")


@pytest.mark.parametrize("name", GEO_NAMES)
def test_row_comparator_rejects_every_corruption(name):
    geo = mt.GEO[name]

    def want(case, exp):
        if exp["rows"] < 3 or exp["v"][-1] != 0 or case["k"] < 1:
            return False
        c = exp["cells"][0, :exp["nc"][0]]
        return (c <= case["k"]).any() and (c > case["k"]).any()

    case, exp = _a_case(name, want)
    k = case["k"]
    good = mt.as_device_rows(geo, exp)
    assert mt.compare_rows(geo, case, exp, good) == []
    c = exp["cells"][0, :exp["nc"][0]]
    low, high = int(np.argmax(c <= k)), int(np.argmax(c > k))
    for what, change in [
        ("cell at most maxED, one higher", lambda d: d["cells"][0].__setitem__(low, c[low] + 1)),
        ("cell above maxED read as maxED", lambda d: d["cells"][0].__setitem__(high, k)),
        ("verdict of a valid row", lambda d: d["verdict"].__setitem__(0, 0)),
        ("verdict of the invalid row", lambda d: d["verdict"].__setitem__(len(d) - 1, 1)),
        ("RAC one to the left", lambda d: d["rac"].__setitem__(0, d["rac"][0] - 1)),
        ("RAC one to the right", lambda d: d["rac"].__setitem__(1, d["rac"][1] + 1)),
    ]:
        d = good.copy()
        change(d)
        assert mt.compare_rows(geo, case, exp, d) != [], what
    assert mt.compare_rows(geo, case, exp, good[:-1]) != [], "a missing row"
    d = good.copy()
    d["cells"][0][high] = c[high] + 3  # above maxED on both sides: not a finding
    if high + exp["fc"][0] != 1:       # (unless it is the diagonal cell, which the score repeats)
        assert mt.compare_rows(geo, case, exp, d) == []
    d = good.copy()
    assert mt.compare_rows(geo, case, exp, d, ovgl=[1 - int(x) for x in d["ovgl"]]) != [], "onlyVerticalGapsLeft"


@pytest.mark.parametrize("narrow", [True, False], ids=["narrow", "wide"])
def test_walk_comparator_rejects_every_corruption(narrow):
    cases, exps, _, _ = mt.trace_cases(narrow)
    exp = next(e for e in exps if e["n"] >= 2 and int(e["walks"][0][2]) >= 3)
    assert mt.compare_walks(exp, exp["n"], exp["valid"], exp["walks"]) == []
    for what, idx, delta in [("run length", (0, 5), 4), ("run operation", (0, 4), 1), ("number of runs", (1, 2), 1), ("end row", (0, 1), 1),
                             ("start row", (1, 0), 1), ("flags", (0, 3), 2)]:
        w = exp["walks"].copy()
        w[idx] += delta
        assert mt.compare_walks(exp, exp["n"], exp["valid"], w) != [], what
    assert mt.compare_walks(exp, exp["n"] - 1, exp["valid"], exp["walks"]) != []
    assert mt.compare_walks(exp, exp["n"], exp["valid"] + 1, exp["walks"]) != []


def test_word_comparator_rejects_one_bit():
    sources, q = mt.word_queries()
    exp = mt.plain_words(sources, q)
    kinds = np.bincount(q[:, 0], minlength=len(mt.WORD_KINDS))
    print("word queries:", ", ".join(f"{w['name']} {n}" for w, n in zip(mt.WORD_KINDS, kinds)))
    assert (kinds > 0).all() and set(q[:, 2]) == set(range(96)) and set(q[:, 3]) == set(mt.WORD_LENGTHS)
    assert len(mt.compare_words(exp, exp.copy())) == 0
    for at, bit in [(0, 0), (len(exp) // 2, 21), (len(exp) - 1, 63)]:
        d = exp.copy()
        d[at] ^= np.uint64(1) << np.uint64(bit)
        assert mt.compare_words(exp, d).tolist() == [at]
    # the reference itself, on a word small enough to write down: X = "ACG", nucleotide C, LEFT 3, BLOCK 4
    L = mt.lib()
    assert L.gt_match_word(b"ACG", 3, 3, 4, 0, ord("C")) == 0b010111
    assert L.gt_match_word(b"ACG", 3, 3, 4, 1, ord("C")) == 0b1 and L.gt_match_word(b"ANG", 3, 3, 4, 0, ord("N")) == 0b111


def test_plain_reference_on_a_matrix_small_enough_to_write_down():
    """X = ACGT against Y = AGGTA at maxED 1, fixed start, worked by hand: rows 0 1 2 3 4 / 1 0 1 2 3 / 2 1 1 1 2 / 3 2 2 1 2 / 4 3 3 2 1 /
    5 4 4 3 2; the rightmost active column 1, 2, 3, 3 (a walk: the diagonal step costs one), 4, none"""
    exp = mt.plain_rows(dict(x=b"ACGT", y=b"AGGTA", init=[0], k=1))
    assert exp["rows"] == 5 and exp["v"].tolist() == [1, 1, 1, 1, 0]
    assert [exp["cells"][r, :exp["nc"][r]].tolist() for r in range(5)] == [[1, 0, 1], [1, 1, 1], [2, 1, 2], [2, 1], [2]]
    assert exp["rac"].tolist() == [2, 3, 3, 4, -2 ** 31] and exp["ev"].tolist() == [2, 2, 0, 2, 0]
    walks, _ = mt.plain_walks(dict(x=b"ACGT", y=b"AGGTA", k=1, nzeros=1), narrow=True)
    assert walks["n"] == 1 and walks["walks"][0][:5].tolist() == [4, 0, 1, 0, (4 << 2) | 0]


def test_probe_compiles_with_the_library_flags(tmp_path):
    out = mt.compile_probe(str(tmp_path / "matrix_probe"))
    import os
    assert os.path.getsize(out) > 0
