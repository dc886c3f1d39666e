"""The read loop shared by rb_align, rb_markers and rb_locs (rowbowt_amd/csrc/cli_pipeline.hpp), CPU only: the driver over a
real InputSource with fake stages (tests/cpp/cli_pipeline_check.cpp, which checks the order of the calls as they happen),
built once under AddressSanitizer + UBSan and once under ThreadSanitizer.  stdout must be one line per record, in file order,
whatever the window, the batch and the number of formatting threads."""
import gzip
import os
import subprocess

import pytest

from kseq_model import kseq_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZERS = {"asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "tsan": ["-fsanitize=thread"]}
HUGE = 1 << 30


@pytest.fixture(scope="module", params=sorted(SANITIZERS))
def pipeline(request, tmp_path_factory):
    exe = tmp_path_factory.mktemp("pl_" + request.param) / "cli_pipeline_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread"] + SANITIZERS[request.param] +
                          [os.path.join(ROOT, "tests", "cpp", "cli_pipeline_check.cpp"), "-o", str(exe), "-lz"])

    def run(mode, path, window, batch, threads, exit_code=0):
        p = subprocess.run([str(exe), mode, str(path), str(window), str(batch), str(threads)], capture_output=True, timeout=120)
        assert p.returncode == exit_code, (mode, window, batch, threads, p.stdout[-200:], p.stderr[-1500:])
        stats = [l for l in p.stderr.decode().splitlines() if l.startswith("rc=")]
        assert len(stats) == 1, p.stderr[-1500:]
        st = dict(kv.split("=") for kv in stats[0].split())
        st["window_sizes"] = [int(v) for v in st["window_sizes"].split(",") if v]
        return p.stdout, {k: v if k == "window_sizes" else int(v) for k, v in st.items()}, p.stderr.decode()
    return run


def fastq(n, m=9):
    """n records of m bases, 15 + 2 m bytes each: (name, sequence) pairs and the file's bytes"""
    recs = [(b"r%06d" % i, (b"ACGT" * m)[i % 4:i % 4 + m]) for i in range(n)]
    return recs, b"".join(b"@" + name + b" c\n" + seq + b"\n+\n" + b"I" * m + b"\n" for name, seq in recs)


def lines(recs):
    return b"".join(name + b" %d\n" % len(seq) for name, seq in recs)


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("pl_in")
    out = {}
    for name, n in (("small", 400), ("big", 12000), ("wide", 70000), ("one", 1), ("empty", 0)):
        recs, blob = fastq(n)
        (d / (name + ".fq")).write_bytes(blob)
        out[name] = (d / (name + ".fq"), recs)
    (d / "blank_tail.fq").write_bytes((d / "small.fq").read_bytes() + b"\n")
    out["blank_tail"] = (d / "blank_tail.fq", out["small"][1])
    for name in ("small", "big"):
        (d / (name + ".fq.gz")).write_bytes(gzip.compress((d / (name + ".fq")).read_bytes(), 1))
        out[name + "_gz"] = (d / (name + ".fq.gz"), out[name][1])
    return out


def test_stdout_is_one_line_per_record_in_file_order(pipeline, inputs):
    """windows of 1 KB, 64 KB and larger than the file; batches of 1, 7 (dividing no window), a window's size and larger; 1, 3 and 16
    threads.  A batch is split over min(threads, ceil(N / 4096), 64) workers, so only batches of more than 4096 reads are split at
    all: the 12 000 reads of `big` in one batch make three slices, the 70 000 of `wide` sixteen.  Batches of one read run on `small`
    (400 reads; every batch costs a thread and 200 us of the fake query)."""
    for name, cases in (("small", ((1 << 10, 1, 1), (1 << 10, 7, 3), (1 << 10, "window", 16), (1 << 10, HUGE, 3), (1 << 16, 1, 3), (1 << 16, 7, 1),
                                   (1 << 16, HUGE, 16))),
                        ("big", ((1 << 16, 7, 3), (1 << 16, "window", 16), (1 << 16, HUGE, 1), (HUGE, 4100, 3), (HUGE, HUGE, 1), (HUGE, HUGE, 3),
                                 (HUGE, HUGE, 16)))):
        path, recs = inputs[name]
        for window, batch, threads in cases:
            if batch == "window":
                _, st, _ = pipeline("run", path, window, HUGE, 1)
                batch = st["window_sizes"][0]
                assert st["windows"] > 5 and batch == st["window_sizes"][1]
            out, st, _ = pipeline("run", path, window, batch, threads)
            assert out == lines(recs), (name, window, batch, threads)
            assert st["rc"] == -1 and sum(st["window_sizes"]) == len(recs) and st["batches"] == sum(-(-w // batch) for w in st["window_sizes"])
            assert (st["windows"] == 1) == (window > os.path.getsize(path))
            if batch == 7:
                assert st["window_sizes"][0] % 7
            # every batch but a window's first is queried ahead, on another thread
            assert st["ahead"] == st["batches"] - sum(1 for w in st["window_sizes"] if w)
            assert st["pieces_held"] <= st["max_window_pieces"]
            if window == HUGE and batch == HUGE:
                assert st["max_window_pieces"] == min(threads, 3)
    path, recs = inputs["wide"]
    out, st, _ = pipeline("run", path, HUGE, HUGE, 16)
    assert out == lines(recs) and st["max_window_pieces"] == 16 and st["windows"] == 1
    out, st, _ = pipeline("run", path, 1 << 18, 5000, 3)     # a batch of two slices and one of one per window, the pool recycled from window to window
    assert out == lines(recs) and st["windows"] > 5 and st["pieces_held"] <= st["max_window_pieces"] == 3


def test_shard_by_slice_pieces_and_ready_texts_keep_file_order(pipeline, inputs):
    """the two other ways a tool fills the pool: rb_align's shards x slices through format_ranges (three shards here; batches of one and
    two reads leave shards empty, shard 0 among them, whose slice still runs on the caller) and a text made elsewhere through
    PiecePool::put (rb_markers --device-format), alternating from batch to batch"""
    for name, cases in (("small", ((1 << 10, 1, 3), (1 << 10, 2, 1), (1 << 10, 7, 3), (1 << 16, HUGE, 16))),
                        ("big", ((1 << 16, 500, 3), (HUGE, 4100, 3), (HUGE, HUGE, 16))), ("wide", ((HUGE, HUGE, 16), (1 << 18, 5000, 3)))):
        path, recs = inputs[name]
        for window, batch, threads in cases:
            out, st, _ = pipeline("shards", path, window, batch, threads)
            assert out == lines(recs), (name, window, batch, threads)
            assert st["rc"] == -1 and st["pieces_held"] <= st["max_window_pieces"]
            if window == HUGE and batch == HUGE:      # one batch, ticket 0: three shards of min(threads, ceil(N / 4096)) slices
                assert st["max_window_pieces"] == 3 * min(threads, -(-len(recs) // 4096))
            if (window, batch) == (HUGE, 4100):       # 12 000 reads: 6 pieces, a ready text, 3 pieces
                assert st["max_window_pieces"] == 3 * 2 + 1 + 3 * 1


def test_empty_file_one_record_empty_last_window_and_gzip(pipeline, inputs):
    for name in ("empty", "one"):
        path, recs = inputs[name]
        for window, batch, threads in ((1 << 10, 1, 1), (HUGE, 7, 3)):
            out, st, _ = pipeline("run", path, window, batch, threads)
            assert out == lines(recs) and st["rc"] == -1 and st["windows"] == 1 and st["batches"] == len(recs)
    # (a blank line behind the last record: the window that holds it finds the end of the file and no record)
    path, recs = inputs["blank_tail"]
    out, st, _ = pipeline("run", path, 50 * (os.path.getsize(path) // len(recs)), 7, 3)
    assert st["window_sizes"] == [50] * 8 + [0] and st["rc"] == -1
    assert out == lines(recs)
    for name, cases in (("small_gz", ((1 << 10, 7, 1), (1 << 10, 1, 3))), ("big_gz", ((1 << 16, 500, 3), (1 << 20, HUGE, 16)))):   # (zlib's path fills a buffer of the window's size)
        path, recs = inputs[name]
        for window, batch, threads in cases:
            out, st, _ = pipeline("run", path, window, batch, threads)
            assert out == lines(recs) and st["rc"] == -1 and (st["windows"] > 5) == (window < 1 << 20)


def test_format_that_throws_leaves_once_every_thread_has_returned(pipeline, inputs):
    """`format` throws on batch 3 of window 2 with the query of batch 4 and the scan of window 3 in flight and window 1 being written:
    the driver rethrows after joining all three (a thread left behind would touch what the program then reuses: ThreadSanitizer and
    AddressSanitizer see that), windows 0 and 1 are on stdout, window 2's text is dropped"""
    path, recs = inputs["big"]
    for threads in (1, 3):
        out, st, _ = pipeline("throw", path, 1 << 16, 100, threads)
        w = st["window_sizes"]
        assert len(w) == 3 and w[2] > 500
        assert out == lines(recs[:w[0] + w[1]])
        assert st["batches"] == -(-w[0] // 100) + -(-w[1] // 100) + 5     # batches 0..4 of window 2 were prepared and queried


def test_input_errors_come_back_as_the_scanners_code(pipeline, inputs, tmp_path):
    """a truncated quality string: -2 after the records before it, and the tools' exit through exit_on_input_error (exit 1 with kseq's
    message); a BGZF file with a damaged block: -3 likewise"""
    _, blob = fastq(3000)
    data = blob[:len(blob) - 5]
    want, want_rc = kseq_model(data)
    assert want_rc == -2 and len(want) == 2999
    f = tmp_path / "trunc.fq"
    f.write_bytes(data)
    for window, batch, threads in ((1 << 12, 7, 3), (HUGE, 1000, 1)):
        out, st, err = pipeline("run", f, window, batch, threads, exit_code=1)
        assert st["rc"] == -2 and out == lines(want) and err.endswith("ERROR: truncated quality string\n")
    from test_fastx_host import bgzf_bytes
    z = bytearray(bgzf_bytes(blob, block=4000))
    pos = 0
    for _ in range(10):     # the eleventh block
        pos += (z[pos + 16] | (z[pos + 17] << 8)) + 1
    z[pos + 30] ^= 0x5A
    bad = tmp_path / "bad.fq.gz"
    bad.write_bytes(bytes(z))
    all_recs = fastq(3000)[0]
    for window, batch in ((9000, 7), (HUGE, HUGE)):
        out, st, err = pipeline("run", bad, window, batch, 3, exit_code=1)
        assert st["rc"] == -3 and err.endswith("ERROR: error reading stream\n")
        got = out.split(b"\n")[:-1]
        # (the record the bad block cuts may come out shortened, as from kseq_read when gzread fails inside a sequence)
        assert 10 * 4000 // 40 - 5 <= len(got) < len(all_recs) and got[:-1] == lines(all_recs).split(b"\n")[:len(got) - 1]


def test_sequential_mode_alternates_prepare_and_query_and_writes_nothing(pipeline, inputs):
    """run_in_sequence (rb_markers --tally): the program prints the lines its `query` collected after the driver has returned, so
    anything the driver wrote would show as extra bytes"""
    path, recs = inputs["big"]
    for window, batch in ((1 << 16, 7), (1 << 10, HUGE), (HUGE, 5000)):
        out, st, _ = pipeline("seq", path, window, batch, 3)
        assert out == lines(recs) and st["rc"] == -1 and st["ahead"] == 0
        assert st["batches"] == sum(-(-w // batch) for w in st["window_sizes"])
    path, recs = inputs["empty"]
    out, st, _ = pipeline("seq", path, 1 << 10, 7, 1)
    assert out == b"" and st["batches"] == 0
