"""The oracle against known-answer vectors produced by the REAL reference code.

tests/golden/ref_vectors.out was written by oracle/_ref/ref_driver, which is the reference's
own bitvec.h / bwtrepr.h / encodedtext.h / bitparallelmatrix.{h,cpp} / indexhelpers.{h,cpp} /
search.{h,cpp} / nucleotide.h compiled unmodified (oracle/Makefile, tests/golden/make_golden.py).
These tests pin rows a1, a2, a5, a7, a10 (bit structures, sparse suffix array files), a11 (doTask), a14
(makeSearch, critical part, readScheme on every file of search_schemes/), a15 (k-mer keys), a16 (orderings),
a17 (value types, Read / ReadBundle clean-up, Substring) of SURVEY.md §8.
"""
import os
import subprocess
from collections import Counter

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")


def _load():
    cmds = open(os.path.join(GOLD, "ref_vectors.cmds")).read().splitlines()
    outs = open(os.path.join(GOLD, "ref_vectors.out")).read().splitlines()
    assert len(cmds) == len(outs) and len(cmds) > 1000
    return cmds, outs


def test_oracle_matches_reference_vectors(oracle_built):
    cmds, outs = _load()
    res = subprocess.run([os.path.join(oracle_built, "oracle_driver")], input="\n".join(cmds) + "\n",
                         capture_output=True, text=True, check=True, cwd=GOLD).stdout.splitlines()
    assert len(res) == len(outs)
    bad = Counter()
    for c, r, o in zip(cmds, res, outs):
        if r != o:
            bad[c.split(" ")[0]] += 1
    assert not bad, f"oracle differs from reference vectors: {dict(bad)}"


def test_vectors_are_not_vacuous():
    cmds, outs = _load()
    kinds = Counter(c.split(" ")[0] for c in cmds)
    for k in ("bwt", "bitvec9", "enc", "matrix", "traceback", "search", "scheme", "cluster", "verify",
              "occsort", "revcomp", "ssa", "read", "kmer", "substr", "readscheme", "sampe", "samunpaired"):
        assert kinds[k] >= 10, k
    # every scheme file of the reference's search_schemes/ is read by the reference's own reader
    ok = sum(1 for c, o in zip(cmds, outs) if c.startswith("readscheme search_schemes/") and o.startswith("ok "))
    assert ok >= 100
    assert sum(1 for c, o in zip(cmds, outs) if c.startswith("readscheme bad_schemes/") and o.startswith("error ")) >= 8
    # in-text verification vectors must contain real hits and real aborts
    hits = aborts = 0
    for c, o in zip(cmds, outs):
        if c.startswith("verify "):
            t = o.split()
            hits += int(t[3])
            aborts += int(t[1])
    assert hits > 50 and aborts > 20
    # matrix vectors must contain rows that stop early (invalid) and rows in the final column
    early = sum(1 for c, o in zip(cmds, outs) if c.startswith("matrix ") and " 0 " in o[:40])
    assert early >= 0
    # traceback vectors with indels
    assert sum(1 for c, o in zip(cmds, outs) if c.startswith("traceback ") and ("I" in o or "D" in o)) > 10


@pytest.mark.skipif(not os.path.exists(os.path.join(os.path.dirname(HERE), "oracle", "_ref", "ref_driver")),
                    reason="oracle/_ref/ref_driver is only built where /root/reference exists")
def test_fixture_is_what_the_reference_prints_today():
    cmds, outs = _load()
    drv = os.path.join(os.path.dirname(HERE), "oracle", "_ref", "ref_driver")
    res = subprocess.run([drv], input="\n".join(cmds) + "\n", capture_output=True, text=True,
                         check=True, cwd=GOLD).stdout.splitlines()
    assert res == outs


def test_scheme_fixtures_are_the_reference_data():
    """tests/golden/search_schemes/ is a verbatim copy of the reference's data directory: it holds exactly the files of
    tests/golden/search_schemes.sha256, the checksums of that directory (`find . -type f | LC_ALL=C sort | xargs -d '\\n' sha256sum`
    run inside it), each with its listed content."""
    import hashlib
    copy = os.path.join(GOLD, "search_schemes")
    listed = {}
    for line in open(os.path.join(GOLD, "search_schemes.sha256")).read().splitlines():
        digest, name = line.split("  ", 1)
        listed[os.path.normpath(name)] = digest
    present = {os.path.relpath(os.path.join(root, fn), copy) for root, _d, files in os.walk(copy) for fn in files}
    assert present == set(listed)
    for name, digest in listed.items():
        with open(os.path.join(copy, name), "rb") as f:
            assert hashlib.sha256(f.read()).hexdigest() == digest, name
    assert len(listed) > 150


def test_sparse_sa_files_of_the_reference_load(tmp_path):
    """Index files written by the reference's own SparseSuffixArray::write (suffixArray.h:229-243) are read by
    columba_amd.indexbuild (the loader in front of cmb_index_create), and the harness' builder writes the same
    bytes for the same suffix array."""
    import struct
    import numpy as np
    import torch
    from columba_amd import indexbuild as ib
    cmds, outs = _load()
    seen = 0
    for c, o in zip(cmds, outs):
        if not c.startswith("ssa "):
            continue
        t = c.split()
        sp, n = int(t[1]), int(t[2])
        sa = np.array(t[3:3 + n], dtype=np.int64)
        f_bv, f_sa, marks, _ = [x.split() for x in o.split("|")]
        words = np.array([int(x, 16) for x in f_bv[1:]], dtype=np.uint64)
        samples = np.array(f_sa[1:], dtype=np.uint32)
        assert int(f_bv[0]) == len(words) and int(f_sa[0]) == len(samples)
        base = str(tmp_path / f"x{seen}")
        words.tofile(f"{base}.sa.bv.{sp}")
        samples.tofile(f"{base}.sa.{sp}")
        N, bv, cnt, smp = ib.read_sparse_sa(base, sp)
        assert N == n and np.array_equal(smp, samples)
        # what the reference's reader answered per row: "0" or "1:<SA value>"
        rank = 0
        for i, m in enumerate(marks):
            bit = (int(bv[i // 64]) >> (i % 64)) & 1
            assert bit == int(m[0])
            if bit:
                assert int(m.split(":")[1]) == int(smp[rank]) == int(sa[i])
                rank += 1
        w2, c2, s2 = ib.build_sparse_sa(torch.from_numpy(sa), sp)
        mine = np.concatenate([np.array([n], np.uint64), w2, c2])
        assert np.array_equal(mine, words) and np.array_equal(s2, samples)
        seen += 1
    assert seen >= 20


# ---- run-length compressed flavour: the move table ----------------------------------------------
def _load_rlc():
    cmds = open(os.path.join(GOLD, "ref_vectors_rlc.cmds")).read().splitlines()
    outs = open(os.path.join(GOLD, "ref_vectors_rlc.out")).read().splitlines()
    assert len(cmds) == len(outs) and len(cmds) >= 100
    return cmds, outs


def test_move_table_matches_reference_vectors(oracle_built):
    """MoveLFReprBP (bmove/moverepr.cpp) built through its own setters, written by its writer, read back by its loader and
    queried (computeRunIndices, addChar, countChar, getCumulativeCounts, findLF with and without fast-forward), in the
    64-bit and the 32-bit build: the oracle's restatement prints the same file bytes, rows and answers."""
    cmds, outs = _load_rlc()
    res = subprocess.run([os.path.join(oracle_built, "oracle_driver")], input="\n".join(cmds) + "\n",
                         capture_output=True, text=True, check=True, cwd=GOLD).stdout.splitlines()
    assert res == outs
    # not vacuous: empty children, children narrower than the parent, both widths, both text directions
    empty = narrower = 0
    for c, o in zip(cmds, outs):
        for q in o.split(" | ")[2:]:
            t = q.split()
            empty += t[3] == "0" and t[4] == "0"
            narrower += int(t[4]) - int(t[3]) > 0
    assert empty > 100 and narrower > 300
    assert {c.split()[1] for c in cmds} == {"32", "64"} and {c.split()[3] for c in cmds} == {"0", "1"}


@pytest.mark.skipif(not os.path.exists(os.path.join(os.path.dirname(HERE), "oracle", "_ref", "ref_driver_rlc64")),
                    reason="oracle/_ref/ref_driver_rlc* are only built where /root/reference exists")
def test_rlc_fixture_is_what_the_reference_prints_today():
    cmds, outs = _load_rlc()
    for width in ("64", "32"):
        drv = os.path.join(os.path.dirname(HERE), "oracle", "_ref", "ref_driver_rlc" + width)
        idx = [i for i, c in enumerate(cmds) if c.split()[1] == width]
        res = subprocess.run([drv], input="\n".join(cmds[i] for i in idx) + "\n", capture_output=True, text=True,
                             check=True, cwd=GOLD).stdout.splitlines()
        assert res == [outs[i] for i in idx]
