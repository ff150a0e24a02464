"""FASTQ chunks parsed on the device (cmb_reads_*, csrc/reads.hip, csrc/dev_reads.hpp) against Reader of include/columba_amd_io.hpp,
which is the parser's specification: tests/reader_driver.cpp prints what Reader returns, call for call and record for record, and every
case below is held to that output (never to another device run).

The Python side reads a file as Reader's caller would: one parse per getNextChunk call, the window being the rest of the file, the
next window beginning at `consumed`.  Windows that end inside a file (final = 0) have a test of their own, and DeviceReader — the C++
class that cuts a file into windows — runs through the same driver built with -DREADER_DEVICE.

Run with `pytest -m gpu` on an MI355X.
"""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import columba_amd as ca
from columba_amd import indexbuild as ib
from columba_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINK = ["-L", os.path.join(ROOT, "columba_amd"), "-lcolumba_amd", "-lz", "-Wl,-rpath," + os.path.join(ROOT, "columba_amd"), "-Wl,-rpath,/opt/rocm/lib"]
KERNELS = ("k_rd_count", "k_rd_place", "k_rd_classify", "k_rd_starts", "k_rd_fields", "k_rd_gather")


# ------------------------------------------------------------------------------------------------ Reader, through its driver
@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    ca.build_library()
    tmp = str(tmp_path_factory.mktemp("reader_driver"))
    src, inc = os.path.join(ROOT, "tests", "reader_driver.cpp"), os.path.join(ROOT, "include")
    host, dev = os.path.join(tmp, "reader_driver"), os.path.join(tmp, "reader_driver_device")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", inc, src, "-o", host, "-lz"])
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-DREADER_DEVICE", "-I", inc, src, "-o", dev] + LINK)
    return {"tmp": tmp, "host": host, "device": dev}


def _driver_calls(exe, path, n, calls):
    """([(return value, [(identifier, read, quality)])] per call, the exception's message or None)"""
    out = subprocess.run([exe, path, str(n), str(calls)], stdout=subprocess.PIPE, check=False).stdout
    res, pos, error = [], 0, None
    while pos < len(out):
        nl = out.index(b"\n", pos)
        head = out[pos:nl].split(b" ", 1)
        pos = nl + 1
        if head[0] == b"C":
            res.append((int(head[1].split()[0]), []))
        elif head[0] == b"R":
            a, b, c = (int(x) for x in head[1].split())
            res[-1][1].append((out[pos:pos + a], out[pos + a:pos + a + b], out[pos + a + b:pos + a + b + c]))
            assert out[pos + a + b + c:pos + a + b + c + 1] == b"\n"
            pos += a + b + c + 1
        else:
            assert head[0] == b"E", head
            error = head[1].decode()
    for ret, recs in res:
        assert ret == (1 if recs else 0)  # (Reader::getNextChunk returns !chunk.empty())
    return res, error


def _device_calls(parser, data, n, calls):
    """the same calls through the device parser: the rest of the file is the window of every call"""
    res, pos, error = [], 0, None
    for _ in range(calls):
        try:
            p = parser.parse(data[pos:], n, True)
        except ca.CmbError as e:
            # (a window of its own that begins with '>' is refused as FASTA; inside a window the same record is a bad FASTQ record)
            assert e.code == ca.CMB_ERR_INVALID or (e.code == ca.CMB_ERR_UNSUPPORTED and data[pos:pos + 1] == b">"), e
            error = str(e)
            break
        recs = p.records()
        assert len(recs) == p.n_records
        res.append((1 if recs else 0, recs))
        pos += p.consumed
        assert pos <= len(data)
    return res, error


def _write(tmp, name, data):
    path = os.path.join(tmp, name)
    with open(path, "wb") as f:
        f.write(data)
    return path


def _same_calls(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for c, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w[0] and len(g[1]) == len(w[1]), (what, "call", c, g[0], w[0], len(g[1]), len(w[1]))
        for i, (x, y) in enumerate(zip(g[1], w[1])):
            assert x == y, (what, "call", c, "record", i, x[0][:60], y[0][:60], len(x[1]), len(y[1]), len(x[2]), len(y[2]))


# ------------------------------------------------------------------------------------------------ hand-made files
def _record(i, length, rng, eol=b"\n"):
    read = bytes(rng.choice(np.frombuffer(b"ACGTN", np.uint8), length))
    qual = bytes(rng.integers(33, 74, length).astype(np.uint8))
    return b"@r%d len=%d" % (i, length) + eol + read + eol + b"+" + eol + qual + eol


def _mixed_lengths():
    rng = np.random.default_rng(3)
    lengths = [1, 600, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 149, 150, 151, 255, 256, 257, 480, 481, 599] + [int(x) for x in rng.integers(1, 601, 36)]
    return b"".join(_record(i, n, rng) for i, n in enumerate(lengths))


def _long_read():
    rng = np.random.default_rng(4)
    return _record(0, 150, rng) + _record(1, 70_000, rng) + _record(2, 33, rng) + _record(3, 4097, rng)


THREE = b"@a x\nACGT\n+\nIIII\n@b\nAC\n+a\nI#\n@c\nT\n+\nI\n"
EDGE_CASES = {
    "lf": THREE,
    "crlf": THREE.replace(b"\n", b"\r\n"),
    "blank_and_cr_led_lines": b"\n\r\n\rjunk\n@a\nACGT\n+\nIIII\n\n\r\n@b\nAC\n+\nII\n\rjunk @x\n\n@c\nA\n+\nI\n\n\n",
    "blank_line_inside_a_record": b"@a\nACGT\n\nIIII\n@b\nAC\n+\n\n@c\nT\n+\nI\n",
    "quality_begins_with_at_and_plus": b"@a\nACGT\n+\n@III\n@b\nACGT\n+\n+III\n@c\nAC\n+\n@@\n",
    "identifiers_with_spaces_and_tabs": b"@read 1\tdesc x  y\nACGT\n+read 1\nIIII\n@ lead\nAC\n+\nII\n@\nA\n+\nI\n@t\t\nAG\n+\nII\n",
    "several_trailing_cr": b"@a\r\r\nAC\r\r\n+\nII\r\n@b \r\nA\r\n+\r\nI\r\r\r\n",
    "mixed_lengths": _mixed_lengths(),
    "long_read": _long_read(),
    "no_final_newline": THREE[:-1],
    "no_final_newline_crlf": THREE.replace(b"\n", b"\r\n")[:-2],
    "final_record_of_1_line": THREE + b"@e",
    "final_record_of_1_line_nl": THREE + b"@e\n",
    "final_record_of_2_lines": THREE + b"@e\nTT",
    "final_record_of_2_lines_nl": THREE + b"@e\nTT\n",
    "final_record_of_3_lines": THREE + b"@e\nTT\n+",
    "final_record_of_3_lines_nl": THREE + b"@e\nTT\n+\n",
    "final_cr_without_newline": THREE + b"\r",
    "empty_read_in_the_middle": b"@a\nAC\n+\nII\n@b\nA\n+\nI\n@c\n\n+\nII\n@d\nACG\n+\nIII\n@e\nT\n+\nI\n",
    "empty_read_first": b"@c\n\n+\nII\n@d\nACG\n+\nIII\n@e\nT\n+\nI\n",
    "empty_read_crlf": b"@a\r\nAC\r\n+\r\nII\r\n@c\r\n\r\n+\r\nII\r\n@d\r\nACG\r\n+\r\nIII\r\n",
    "two_empty_reads": b"@a\nAC\n+\nII\n@c\n\n+\nII\n@c2\n\r\n+\nII\n@d\nACG\n+\nIII\n",
    "empty_file": b"",
    "blank_lines_only": b"\n\r\n\n\r \n",
    "record_without_at": b"@a\nAC\n+\nII\nXb\nAC\n+\nII\n@c\nA\n+\nI\n",
    "fasta_record_in_a_fastq_file": b"@a\nAC\n+\nII\n>b\nAC\n@c\nA\n+\nI\n",
}


@pytest.fixture(scope="module")
def parser(drivers):
    p = ca.ReadParser()
    yield p
    p.close()


@pytest.mark.parametrize("name", sorted(EDGE_CASES))
def test_edge_cases_equal_reader(drivers, parser, name):
    data = EDGE_CASES[name]
    path = _write(drivers["tmp"], name + ".fq", data)
    n_lines = data.count(b"\n") + 1
    for n in (1, 3, 100):
        calls = min(n_lines, (n_lines // 4) // n + 8) if n > 1 else min(n_lines // 2 + 4, 80)
        want, want_error = _driver_calls(drivers["host"], path, n, calls)
        got, got_error = _device_calls(parser, data, n, calls)
        _same_calls(got, want, (name, n))
        assert (got_error is None) == (want_error is None), (name, n, got_error, want_error)
        if want_error:
            assert "doesn't appear to be in FastQ format" in want_error and ("does not begin with '@'" in got_error or "FASTA" in got_error)
    if name not in ("record_without_at", "fasta_record_in_a_fastq_file"):
        assert want_error is None
        assert sum(len(r) for _, r in want) >= {"empty_file": 0, "blank_lines_only": 0}.get(name, 1)


@pytest.mark.parametrize("name", ["crlf", "blank_and_cr_led_lines", "long_read", "final_record_of_2_lines", "empty_read_in_the_middle",
                                  "empty_read_first", "empty_file", "record_without_at"])
def test_device_reader_class_equals_reader(drivers, name):
    """DeviceReader (windows sized from the chunk, grown for the 70 000-character read, the tail carried over) through the same driver"""
    path = _write(drivers["tmp"], name + ".fq", EDGE_CASES[name])
    for n in (2, 100):
        want, want_error = _driver_calls(drivers["host"], path, n, 8)
        got, got_error = _driver_calls(drivers["device"], path, n, 8)
        _same_calls(got, want, (name, n))
        assert got_error == want_error


def test_fasta_files_keep_the_host_reader(drivers, parser):
    data = b">s1 d\nACGT\nAC\n>s2\nTTT\n"
    with pytest.raises(ca.CmbError) as e:
        parser.parse(data, 10, True)
    assert e.value.code == ca.CMB_ERR_UNSUPPORTED and "FASTA" in str(e.value)
    with pytest.raises(ca.CmbError) as e:
        parser.parse(b"\n\r\n" + data, 10, False)
    assert e.value.code == ca.CMB_ERR_UNSUPPORTED
    assert parser.parse(b"", 10, True).n_records == 0  # (the handle works on)
    path = _write(drivers["tmp"], "reads.fa", data)
    want, _ = _driver_calls(drivers["host"], path, 10, 2)
    got, _ = _driver_calls(drivers["device"], path, 10, 2)
    assert want[0][1] == [(b">s1 d", b"ACGTAC", b"*"), (b">s2", b"TTT", b"*")]
    _same_calls(got, want, "fasta")


# ------------------------------------------------------------------------------------------------ windows and max_records
@pytest.fixture(scope="module")
def forty(drivers):
    rng = np.random.default_rng(17)
    recs = [_record(i, int(rng.integers(1, 40)), rng, b"\r\n" if i % 5 == 0 else b"\n") for i in range(40)]
    recs[7] = b"\n\r\n" + recs[7]      # blank lines in front of records, in the middle of the cuts too
    recs[21] = b"\n" + recs[21]
    data = b"".join(recs)
    ends = np.cumsum([len(r) for r in recs])
    path = _write(drivers["tmp"], "forty.fq", data)
    want, error = _driver_calls(drivers["host"], path, 100, 2)
    assert error is None and len(want[0][1]) == 40 and want[1] == (0, [])
    return {"data": data, "ends": [int(e) for e in ends], "records": want[0][1]}


def test_windows_that_end_inside_a_record(forty, parser):
    """every prefix that ends inside records 20 and 21, final = 0: exactly the records that lie wholly inside it, consumed = the end of
    the last of them; the rest of the file from there with final = 1 gives the other records"""
    data, ends, records = forty["data"], forty["ends"], forty["records"]
    cuts = list(range(ends[19], ends[21] + 1))
    assert 60 <= len(cuts) <= 200
    for cut in cuts:
        whole = sum(1 for e in ends if e <= cut)
        p = parser.parse(data[:cut], 1000, False)
        assert (p.n_records, p.consumed, p.stop) == (whole, ends[whole - 1], ca.READS_STOP_WINDOW), cut
        assert p.records() == records[:whole], cut
        q = parser.parse(data[p.consumed:], 1000, True)
        assert q.records() == records[whole:], cut
        assert (q.consumed, q.stop) == (len(data) - p.consumed, ca.READS_STOP_WINDOW), cut
    # the same cuts as the end of the FILE: the cut record is taken with what there is of it
    read_at = data.index(b"\n", ends[19]) + 1
    cut = read_at + 1
    p = parser.parse(data[:cut], 1000, True)
    assert (p.n_records, p.consumed, p.stop) == (21, cut, ca.READS_STOP_WINDOW) and p.records()[:20] == records[:20]
    assert p.records()[20] == (records[20][0], records[20][1][:1], b"")
    # ... and cut inside its identifier line it has no read: it ends the chunk and is consumed
    p = parser.parse(data[:ends[19] + 3], 1000, True)
    assert (p.n_records, p.consumed, p.stop) == (20, ends[19] + 3, ca.READS_STOP_EMPTY_READ) and p.records() == records[:20]


def test_max_records(forty, parser):
    data, ends, records = forty["data"], forty["ends"], forty["records"]
    for m, stop in ((1, ca.READS_STOP_MAX_RECORDS), (39, ca.READS_STOP_MAX_RECORDS), (40, ca.READS_STOP_MAX_RECORDS), (41, ca.READS_STOP_WINDOW)):
        for final in (True, False):
            p = parser.parse(data, m, final)
            take = min(m, 40)
            assert (p.n_records, p.consumed, p.stop) == (take, ends[take - 1], stop), (m, final)
            assert p.records() == records[:take]
            assert int(p.offs[take]) == sum(len(r[1]) for r in records[:take]) and int(p.offs[0]) == 0


def test_errors_reach_only_as_far_as_the_chunk(parser):
    data = EDGE_CASES["record_without_at"]
    with pytest.raises(ca.CmbError) as e:
        parser.parse(data, 100, True)
    assert e.value.code == ca.CMB_ERR_INVALID and "record 1 " in str(e.value)
    with pytest.raises(ca.CmbError) as e:
        parser.parse(data, 2, True)
    assert "record 1 " in str(e.value)
    p = parser.parse(data, 1, True)     # the chunk ends in front of the bad record
    assert p.records() == [(b"@a", b"AC", b"II")] and p.stop == ca.READS_STOP_MAX_RECORDS and p.consumed == 11
    # an empty read in front of the bad record ends the chunk there as well; the bad record directly behind an empty-read record is not reached
    p = parser.parse(b"@a\nAC\n+\nII\n@c\n\n+\nII\nXb\nAC\n+\nII\n", 100, True)
    assert p.n_records == 1 and p.stop == ca.READS_STOP_EMPTY_READ and p.consumed == 20
    with pytest.raises(ca.CmbError) as e:
        parser.parse(b"Xb\nAC\n+\nII\n", 100, True)
    assert e.value.code == ca.CMB_ERR_INVALID and "record 0 " in str(e.value)


# ------------------------------------------------------------------------------------------------ the scan across blocks and trips
@pytest.fixture(scope="module")
def twenty_thousand(drivers):
    rng = np.random.default_rng(2024)
    parts = []
    for i in range(20_000):
        if rng.random() < 0.1:
            parts.append((b"\n", b"\r\n", b"\rjunk @%d\n" % i, b"\n\n\r\n")[int(rng.integers(0, 4))])
        parts.append(_record(i, int(rng.integers(20, 120)), rng, b"\r\n" if rng.random() < 0.02 else b"\n"))
    data = b"".join(parts)
    path = _write(drivers["tmp"], "twenty_thousand.fq", data)
    want, error = _driver_calls(drivers["host"], path, 7_000, 4)
    assert error is None and [len(r) for _, r in want] == [7_000, 7_000, 6_000, 0]
    return {"data": data, "path": path, "want": want}


@pytest.mark.parametrize("cap", [1, 3, None])
def test_state_scan_carries_across_blocks_and_trips(twenty_thousand, parser, monkeypatch, capfd, cap):
    monkeypatch.setenv("CMB_VERBOSE", "1")
    if cap:
        monkeypatch.setenv("CMB_TEST_GRID_CAP", str(cap))
    capfd.readouterr()
    got, error = _device_calls(parser, twenty_thousand["data"], 7_000, 4)
    err = capfd.readouterr().err
    assert error is None
    _same_calls(got, twenty_thousand["want"], cap)
    lines = {}
    for k, items, lanes in re.findall(r"\[grid\] (\w+) (\d+) items, (\d+) lanes", err):
        lines.setdefault(k, []).append((int(items), int(lanes)))
    assert sorted(lines) == sorted(KERNELS), sorted(lines)
    assert re.search(r"\[reads\] \d+ bytes, 7000 records: upload [0-9.]+ ms, kernels [0-9.]+ ms, download [0-9.]+ ms", err)
    if cap:
        for k in KERNELS:  # a first, a middle and a last trip in every capped kernel
            assert all(lanes == cap * 256 for _, lanes in lines[k]), (k, lines[k])
            assert max(items for items, _ in lines[k]) >= 3 * cap * 256, (k, lines[k])


def test_device_reader_class_over_many_windows(twenty_thousand, drivers):
    """chunks of 900 records from windows of 64 KiB that grow and carry their tails"""
    want, _ = _driver_calls(drivers["host"], twenty_thousand["path"], 900, 24)
    got, error = _driver_calls(drivers["device"], twenty_thousand["path"], 900, 24)
    assert error is None and sum(len(r) for _, r in want) == 20_000
    _same_calls(got, want, "900 per chunk")


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def small_world(drivers):
    g, _ = synth.genome_rep(seed=41, n=200_000, scale=4.0)
    g = g[:20_000]
    starts = np.array([0, 12_000, 20_000], dtype=np.uint64)
    ix = ib.build_index(g.tobytes(), seq_starts=starts, device="cuda")
    reads = synth.sample_reads(g, 300, 100, seed=12, n_frac=0.01, edit_choices=(0, 1, 2, 4))
    rng = np.random.default_rng(6)
    ids = [f"@read{i}/1 some description\tx" for i in range(len(reads))]
    quals = ["".join(chr(33 + int(q)) for q in rng.integers(0, 41, len(r))) for r in reads]
    fastq = b"".join(i.encode() + b"\n" + r + b"\n+\n" + q.encode() + b"\n" for i, r, q in zip(ids, reads, quals))
    return {"genome": g, "dev": ca.Index(ix), "reads": reads, "ids": ids, "quals": quals, "names": ["chr1", "chr2"], "fastq": fastq}


def test_packed_arrays_feed_batch_and_best_device(small_world, parser):
    """the parser's arrays are the arrays pack_reads / pack_fields make of the lists, the SAM text from them is the text of the list
    route byte for byte, and the copies in HBM hold the bytes of the host views"""
    w = small_world
    p = parser.parse(w["fastq"], 1000, True)
    assert p.n_records == 300 and p.stop == ca.READS_STOP_WINDOW and p.consumed == len(w["fastq"])
    for (buf, offs), fields in ((p.packed, w["reads"]), (p.packed_ids, w["ids"]), (p.packed_quals, w["quals"])):
        want_buf, want_offs = ca.pack_fields(fields)
        assert np.array_equal(offs, want_offs) and np.array_equal(buf, want_buf)
    views = (p.seqs, p.offs, p.ids, p.id_offs, p.quals, p.qual_offs)
    for resident, view in zip(parser.device_tensors(), views):
        assert resident is not None and resident.numel() == view.nbytes
        assert np.array_equal(resident.cpu().numpy(), view.view(np.uint8).reshape(-1))
    st = ca.SearchStrategy("columba", "edit", "dynamic")
    lists = ca.Batch(w["dev"], st, 3, w["reads"])
    packed = ca.Batch(w["dev"], st, 3, packed=p.packed)
    for b in (lists, packed):
        b.want_alignments()
        b.run()
    for xa in (False, True):
        want, _ = lists.sam_device_bytes(w["ids"], w["quals"], w["names"], xa=xa)
        got, _ = packed.sam_device_bytes_packed(p, w["names"], xa=xa)
        assert got == want and got.count(b"\n") >= 300
    lists.close(), packed.close()
    best_lists = ca.BestDevice(w["dev"], st, w["reads"], x=1)
    best_packed = ca.BestDevice(w["dev"], st, x=1, packed=p.packed)
    want, _ = best_lists.sam_device_bytes(w["ids"], w["quals"], w["names"])
    got, _ = best_packed.sam_device_bytes_packed(p, w["names"])
    assert got == want and got.count(b"\n") >= 300
    best_lists.close(), best_packed.close()


# ------------------------------------------------------------------------------------------------ columba_align
@pytest.fixture(scope="module")
def cli(small_world, drivers):
    tmp, w = drivers["tmp"], small_world
    exe = os.path.join(tmp, "columba_align")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "columba_align.cpp"), "-o", exe] + LINK)
    g = w["genome"]
    fa = os.path.join(tmp, "ref.fa")
    with open(fa, "w") as f:
        f.write(">chr1 first\n" + g[:12_000].tobytes().decode() + "\n>chr2\n" + g[12_000:].tobytes().decode() + "\n")
    fq = _write(tmp, "reads.fq", w["fastq"])
    with gzip.open(os.path.join(tmp, "reads.fq.gz"), "wb") as f:
        f.write(w["fastq"])
    rng = np.random.default_rng(9)
    m1, m2 = [], []
    for i in range(120):
        s = int(rng.integers(0, 7_600)) + (12_000 if i % 2 else 0)  # (a fragment of 300 inside chr1 or chr2)
        frag = g[s:s + 300].tobytes()
        m1.append(b"@pair%d/1\n%s\n+\n%s\n" % (i, frag[:100], b"I" * 100))
        m2.append(b"@pair%d/2\n%s\n+\n%s\n" % (i, synth.revcomp(frag[-100:]), b"H" * 100))
    return {"exe": exe, "fa": fa, "fq": fq, "gz": os.path.join(tmp, "reads.fq.gz"), "m1": _write(tmp, "m1.fq", b"".join(m1)),
            "m2": _write(tmp, "m2.fq", b"".join(m2)), "tmp": tmp}


def _align(cli, args, out, device_reader):
    env = dict(os.environ)
    env.pop("CMB_READER_DEVICE", None), env.pop("CMB_READER_HOST", None)
    env["CMB_READER_DEVICE" if device_reader else "CMB_READER_HOST"] = "1"   # (either is named: the test does not depend on the default)
    path = os.path.join(cli["tmp"], out)
    subprocess.check_call([cli["exe"], "-G", cli["fa"], "-o", path] + args, env=env, stderr=subprocess.DEVNULL)
    # (the @PG line quotes the command line, which names the output file)
    return [ln for ln in open(path, "rb").read().split(b"\n") if not ln.startswith(b"@PG")]


@pytest.mark.parametrize("case", ["fq_all", "fq_best", "gz_all", "gz_best", "paired_all"])
def test_columba_align_with_the_device_reader(cli, case):
    args = {"fq_all": ["-f", cli["fq"], "-a", "all", "-e", "3", "-b", "128"], "fq_best": ["-f", cli["fq"], "-b", "77"],
            "gz_all": ["-f", cli["gz"], "-a", "all", "-e", "2", "-XA"], "gz_best": ["-f", cli["gz"], "-b", "128", "-x", "1"],
            "paired_all": ["-f", cli["m1"], "-F", cli["m2"], "-a", "all", "-e", "2", "-O", "fr", "-X", "600", "-b", "50"]}[case]
    want = _align(cli, args, case + "_host.sam", False)
    got = _align(cli, args, case + "_device.sam", True)
    assert got == want
    assert sum(1 for ln in got if ln and not ln.startswith(b"@")) >= (240 if case == "paired_all" else 300)
