"""The retry of the text-occurrence queue (columba_amd.hip: locateAndVerify): when the occurrences of a chunk do not fit the queue's
first size — 48 records per read + 4096 (batchCreateOne) — the queue grows and locate + verification run again, from the counters as
the search left them (`keep`) and with the overflow flag cleared.  The first attempt has already located and verified what fitted, so a
retry that did not restore the counters would report the work of the loop — LF_STEPS and LOCATED_ROWS of k_fmocc and k_verify,
IN_TEXT_STARTED, MATRIX_ROWS, TEXT_BYTES and the CIGAR counter of the verification — too high; one that kept the flag would never end.
Low-complexity text: eight reads of 20 x A match at every position of 1 000 x A, far more often than the first size holds.
  * in-text switch point 4 (the default): the search stays in the index, every text occurrence comes from k_fmocc;
  * in-text switch point 2 000: every range goes to in-text verification at once, the occurrences come from k_verify (Hamming
    distance) and from k_verify_stage + k_traceback (edit distance).
Bar: occurrences and counters bit-exact with the oracle."""
import numpy as np
import pytest

import columba_amd as ca
from columba_amd import indexbuild as ib

pytestmark = pytest.mark.gpu

READS = [b"A" * 20] * 8
TEXT_QUEUE_FIRST_SIZE = 48 * len(READS) + 4096   # (batchCreateOne: b->text)


@pytest.fixture(scope="module")
def poly_a(oracle_built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import oracle_py as op
    ix = ib.build_index(b"A" * 1000, sparseness=4, device="cuda")
    return {sw: (ca.Index(ix, kmer_size=4, in_text_switch=sw), op.OracleIndex(ix, kmer_size=4, switch_point=sw)) for sw in (4, 2000)}


@pytest.mark.parametrize("switch", [4, 2000])
@pytest.mark.parametrize("spec,metric", [("multiple_opt", "edit"), ("kuch1", "hamming")])
def test_text_queue_overflow_is_retried_from_the_saved_counters(poly_a, spec, metric, switch):
    import oracle_py as op
    import schemes_py as sp
    dev, orc = poly_a[switch]
    k = 2
    o_occ, o_off, o_cnt = op.match_batch(orc, op.OracleStrategy(sp.BY_NAME[spec], metric, "dynamic"), k, READS, threads=4)
    # the guards against vacuity, from the oracle alone: the chunk reports more positions than the queue holds at first, and at
    # the high switch point they come from in-text verification
    assert o_cnt["TOTAL_REPORTED_POSITIONS"] > TEXT_QUEUE_FIRST_SIZE, (o_cnt["TOTAL_REPORTED_POSITIONS"], TEXT_QUEUE_FIRST_SIZE)
    assert o_cnt["LOCATED_ROWS"] > TEXT_QUEUE_FIRST_SIZE
    assert (o_cnt["IN_TEXT_STARTED"] > TEXT_QUEUE_FIRST_SIZE) == (switch == 2000), o_cnt["IN_TEXT_STARTED"]
    d_occ, d_off, d_cnt = ca.match_batch(dev, ca.SearchStrategy(spec, metric, "dynamic"), k, READS)
    assert len(o_occ) > 0 and np.array_equal(o_off, d_off)
    for f in ("begin", "end", "distance", "strand"):
        assert np.array_equal(o_occ[f], d_occ[f]), f
    # the counters of test_gpu_parity._compare, net of the in-index duplicates the reference's unstable sort lets through
    names = ["NODE_COUNTER", "IN_TEXT_STARTED", "IMMEDIATE_SWITCH", "SEARCH_STARTED", "EXPANSIONS", "LF_STEPS", "LOCATED_ROWS",
             "TEXT_BYTES", "MATRIX_ROWS", "ABORTED_IN_TEXT_VERIF", "TOTAL_REPORTED_POSITIONS"]
    if metric == "edit":
        names.append("CIGARS_IN_TEXT_VERIFICATION")
    surplus = {"LF_STEPS": o_cnt["SURVIVING_DUP_LF"], "LOCATED_ROWS": o_cnt["SURVIVING_DUP_ROWS"],
               "TOTAL_REPORTED_POSITIONS": o_cnt["SURVIVING_DUP_ROWS"]}
    for n in names:
        assert o_cnt[n] - surplus.get(n, 0) == d_cnt[n], (n, o_cnt[n], surplus.get(n, 0), d_cnt[n])
