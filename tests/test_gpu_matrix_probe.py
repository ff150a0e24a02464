"""The bit-parallel matrices and trace rows of dev_matrix.hpp / dev_trace.hpp against plain dynamic programming, cell by cell.

tests/matrix_probe.hip calls the product's own __device__ functions, one lane per case: every geometry's row (cells, verdict,
rightmost active column, onlyVerticalGapsLeft), every match-word function, and the stored trace rows with the one walk over them.
The cases come from tests/matrixtruth.py (screened with oracle/groundtruth.c until its quotas are full, so the general walk of
racWalk, the block seams and the two implied bits of the narrow rows are met on purpose, not by accident); the comparison is exact:
every cell of at most maxED, every verdict, every RAC, every word bit, every CIGAR run.  A cell above maxED on both sides is not a
finding.  tests/test_matrix_truth.py holds the plain reference to the pinned CPU matrices and checks the comparators.

The probe is compiled once and run once, as one child process; the tests only read its result file.
"""
import subprocess

import numpy as np
import pytest

import matrixtruth as mt

pytestmark = pytest.mark.gpu
PROBE_TIMEOUT = 120  # seconds: the run takes about a second; the rest is process start and the first use of the device


@pytest.fixture(scope="module")
def probe(tmp_path_factory, oracle_built):
    d = tmp_path_factory.mktemp("matrix_probe")
    exe = mt.compile_probe(str(d / "matrix_probe"))
    info = mt.write_case_file(str(d / "cases.bin"))
    # one child process; a non-zero exit, a signal or the timeout fails the fixture and nothing is started again
    run = subprocess.run([exe, str(d / "cases.bin"), str(d / "result.bin")], capture_output=True, text=True, timeout=PROBE_TIMEOUT)
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:])
    return info, mt.read_result_file(str(d / "result.bin"), info)


@pytest.mark.parametrize("name", [g["name"] for g in mt.GEOS])
def test_matrix_rows_equal_plain_dp(probe, name):
    info, res = probe
    geo = mt.GEO[name]
    cases, exps, counts, screened = mt.matrix_cases(name)
    print(f"{name}: {len(cases)} cases, {sum(e['rows'] for e in exps)} rows, {screened} candidates screened; {mt.format_counts(counts)}")
    for q, need in mt.QUOTAS.items():
        assert sum(counts[q].values()) >= need, (name, q, counts[q], "quota not met within the screening cap")
    ovgl = mt.oracle_rows(name) if geo["ref"] else None
    dev = mt.device_rows(name, res, info)
    n_ovgl = 0
    for ci, (case, exp, d) in enumerate(zip(cases, exps, dev)):
        o = None
        if ovgl is not None:
            o = [row[2] if row[0] else None for row in ovgl[ci]]  # (asked on valid rows only)
            n_ovgl += sum(x is not None for x in o)
        bad = mt.compare_rows(geo, case, exp, d, o)
        assert not bad, (name, ci, {k: case[k] for k in ("k", "x", "y", "init", "xoff")}, bad[:5])
    if ovgl is not None:
        print(f"{name}: onlyVerticalGapsLeft equal to the {geo['ref']}-bit CPU matrix on {n_ovgl} valid rows")


def test_match_words_equal_character_comparison(probe):
    info, res = probe
    sources, q = mt.word_queries()
    exp = mt.plain_words(sources, q)
    kinds = np.bincount(q[:, 0], minlength=len(mt.WORD_KINDS))
    print("word queries:", ", ".join(f"{w['name']} {n}" for w, n in zip(mt.WORD_KINDS, kinds)))
    bad = mt.compare_words(exp, res["words"])
    assert len(bad) == 0, [(q[i].tolist(), hex(int(exp[i])), hex(int(res["words"][i]))) for i in bad[:5]]


@pytest.mark.parametrize("narrow", [True, False], ids=["narrow", "wide"])
def test_walks_over_stored_rows_equal_plain_dp(probe, narrow):
    info, res = probe
    cases, exps, counts, screened = mt.trace_cases(narrow)
    print(f"{'narrow' if narrow else 'wide'} rows: {len(cases)} cases, {sum(e['n'] for e in exps)} walks, {screened} candidates screened; "
          f"{mt.format_counts(counts)}")
    for q, need in mt.TRACE_QUOTAS.items():
        assert sum(counts[q].values()) >= need, (narrow, q, counts[q], "quota not met within the screening cap")
    r = res["narrow" if narrow else "wide"]
    for ci, (case, exp) in enumerate(zip(cases, exps)):
        bad = mt.compare_walks(exp, r["n"][ci], r["valid"][ci], r["walks"][ci])
        assert not bad, (ci, {k: case[k] for k in ("k", "x", "y", "nzeros")}, bad[:5])
