"""CPU tests of the compaction's prefix sums: csrc/kernels/results.hip + output.hip compiled for the host, unchanged, under the SIMT shim
of tests/harness/simt/ (tests/harness/compact_prefix_harness.cpp), and k_compact launched directly on synthetic inputs.

A chunk's place in the token stream is its workgroup's own running prefix plus the published totals of the chunks since the
workgroup's previous one, read through one word per group of 64 chunks where the group is complete and through the chunks' own
words where it is not.  The shapes here are the ones at which that arithmetic can go wrong: chunk counts and grids on both sides of
64 and of each other (a range with no multiple of 64 inside, one that starts or ends on one, one with whole groups in the middle, a
grid larger than the batch), a last chunk that is full and one that holds a single pre-token, a chunk whose tokens do not fit the LDS
stage, pre-tokens of 0, 1..4, 7 and 40 tokens so that no two chunks have the same total, empty documents at chunk edges.  The workgroups
of a launch run one after the other under the shim: every total a workgroup needs from a LATER workgroup is unpublished for good and
has to be computed by the one that waits -- at patience 0, 8 and the default.

Expected ids, token CSR and total: a plain sequential loop over the pre-tokens, below."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "harness", "compact_prefix_harness.cpp")
SO = os.path.join(HERE, "harness", "_compact_prefix_harness.so")
CSRC = os.path.join(ROOT, "tokenizers_amd", "csrc")

TOK_ROW, TOK_ONE = 0x80000000, 0x40000000
ROW_CNT_SHIFT, ROW_CNT_MORE = 28, 15

CHUNKS = [1, 2, 63, 64, 65, 128, 129, 200]
GRIDS = [1, 2, 3, 63, 64, 65, 130, 1000]


@pytest.fixture(scope="module")
def harness():
    deps = [SRC, os.path.join(HERE, "harness", "simt", "hip", "hip_runtime.h")] + \
        [os.path.join(CSRC, f) for f in ("kernels/results.hip", "kernels/output.hip", "kernels/scan_util.hip", "kernels.hpp", "overflow_core.hpp", "device_utils.hpp", "tables.hpp")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in deps):
        cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", "-Wno-unused-variable",
               "-I", os.path.join(HERE, "harness", "simt"), "-I", CSRC, SRC, "-o", SO + ".tmp"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        os.replace(SO + ".tmp", SO)
    L = C.CDLL(SO)
    vp = C.c_void_p
    L.cp_run.argtypes = [vp, C.c_int64, vp, C.c_int64, vp, C.c_int64, vp, C.c_int64, C.c_int64, C.c_int, C.c_uint32, C.c_int]
    L.cp_n_tok.restype = C.c_int64
    for f in ("cp_ids", "cp_pt_tokoff", "cp_tok_offsets"):
        getattr(L, f).restype = vp
    for f in ("cp_state_word", "cp_group_word"):
        getattr(L, f).argtypes = [C.c_int64]
        getattr(L, f).restype = C.c_uint64
    L.cp_default_patience.restype = C.c_uint32
    assert L.cp_chunk() == 1024
    return L


_BATCHES = {}


def _batch(n_chunks, last, chunk=1024, stage=2560):
    """tok0 / rows / tmp_ids / doc_pt of (n_chunks - 1) full chunks and one of `last` pre-tokens, and what a sequential loop makes of them"""
    key = (n_chunks, last)
    if key in _BATCHES:
        return _BATCHES[key]
    rng = np.random.default_rng(1000 * n_chunks + last)
    P = (n_chunks - 1) * chunk + last
    kind = rng.integers(0, 100, P)
    cnt = np.where(kind < 70, 1, np.where(kind < 75, 0, np.where(kind < 95, rng.integers(1, 5, P), np.where(kind < 98, 7, 40)))).astype(np.int64)
    fat = n_chunks // 2                                      # one chunk with more tokens than the LDS stage holds
    lo, hi = fat * chunk, min((fat + 1) * chunk, P)
    if hi - lo == chunk:
        cnt[lo:hi:8] = 40
        kind[lo:hi:8] = 99
        assert cnt[lo:hi].sum() > stage
    first_id = rng.integers(0, 1 << 20, P)
    tok0 = np.zeros(P, dtype=np.uint32)
    rows = [[0, 0, 0, 0]]                                    # (row 0: the one every word that names no row loads and drops)
    tmp = [0]
    ids, tok_start = [], np.zeros(P + 1, dtype=np.int64)
    for p in range(P):                                       # THE sequential loop: the tokens of pre-token p follow those of p - 1
        c, i0 = int(cnt[p]), int(first_id[p])
        tok_start[p + 1] = tok_start[p] + c
        mine = [(i0 + j) & 0xFFFFF for j in range(c)]
        ids += mine
        if kind[p] < 70:
            tok0[p] = TOK_ONE | i0
            continue
        tok0[p] = TOK_ROW | len(rows)
        if c <= 4:
            w = mine + [0] * (4 - c)
            w[0] |= c << ROW_CNT_SHIFT
        else:                                                # ids 1.. in tmp_ids[s + 1 ..]
            s = len(tmp) - 1
            w = [i0 | (ROW_CNT_MORE << ROW_CNT_SHIFT), s, c, 0]
            tmp += mine[1:] + [0]
        rows.append(w)
    docs = sorted(set(rng.integers(0, P, max(1, P // 300)).tolist()) | {0})
    edges = [k * chunk for k in range(0, n_chunks + 1, 3) if k * chunk <= P]
    doc_pt = np.array(sorted(docs + edges + edges + [P, P, P]), dtype=np.uint32)      # empty documents at chunk edges and behind the last pre-token
    b = dict(P=P, tok0=tok0, rows=np.array(rows, dtype=np.uint32), tmp=np.array(tmp, dtype=np.uint32), doc_pt=doc_pt,
             ids=np.array(ids, dtype=np.uint32), tok_start=tok_start, tok_offsets=tok_start[doc_pt.astype(np.int64)], chunk_totals=np.add.reduceat(cnt, np.arange(0, P, chunk)))
    _BATCHES[key] = b
    return b


def _run(L, b, grid, patience, want_pt_tokoff=True):
    n_docs = len(b["doc_pt"]) - 1
    T = int(b["tok_start"][-1])
    L.cp_run(b["tok0"].ctypes.data, b["P"], b["rows"].ctypes.data, len(b["rows"]), b["tmp"].ctypes.data, len(b["tmp"]), b["doc_pt"].ctypes.data, n_docs, T,
             grid, patience, 1 if want_pt_tokoff else 0)
    assert L.cp_n_tok() == T
    got_ids = np.ctypeslib.as_array(C.cast(L.cp_ids(), C.POINTER(C.c_uint32)), (max(T, 1),))[:T]
    assert np.array_equal(got_ids, b["ids"])
    got_off = np.ctypeslib.as_array(C.cast(L.cp_tok_offsets(), C.POINTER(C.c_int64)), (n_docs + 1,))
    assert np.array_equal(got_off, b["tok_offsets"])
    if want_pt_tokoff:
        got_pt = np.ctypeslib.as_array(C.cast(L.cp_pt_tokoff(), C.POINTER(C.c_uint32)), (b["P"],))
        assert np.array_equal(got_pt, b["tok_start"][:-1].astype(np.uint32))


def _groups(L, b):
    """(count, sum) of every group word, and the expected sums of the groups wholly inside the batch"""
    tot = b["chunk_totals"]
    n_whole = len(tot) // 64
    words = [L.cp_group_word(g) for g in range(len(tot) // 64 + 1)]
    return [(w >> 56, w & ((1 << 56) - 1)) for w in words], [int(tot[64 * g:64 * g + 64].sum()) for g in range(n_whole)]


@pytest.mark.parametrize("last", [1024, 1], ids=["last-full", "last-single"])
@pytest.mark.parametrize("patience", [0, 8])
@pytest.mark.parametrize("n_chunks", CHUNKS)
def test_every_grid_gives_the_sequential_result(harness, n_chunks, patience, last):
    b = _batch(n_chunks, last)
    for grid in GRIDS:
        _run(harness, b, grid, patience, want_pt_tokoff=(grid % 2 == 1))
        got, exp_sums = _groups(harness, b)
        for g, (count, total) in enumerate(got):
            assert count <= 64, (grid, g, count)                  # only owners add to a group word: never counted twice, whoever helped
            if g < len(exp_sums):
                assert (count, total) == (64, exp_sums[g]), (grid, g)
        for c, t in enumerate(b["chunk_totals"]):                  # every chunk's word holds its total, whoever stored it first
            assert harness.cp_state_word(c) == (1 << 62) | int(t), (grid, c)


@pytest.mark.parametrize("n_chunks,last,grid", [(1, 1, 1), (2, 1024, 1), (65, 1024, 2), (129, 1, 3), (129, 1024, 64), (200, 1024, 65), (200, 1, 130), (200, 1024, 1000), (128, 1024, 63)])
def test_default_patience(harness, n_chunks, last, grid):
    """the product's patience: the long pause before the first help (then the short one), and -- grid 1, or a workgroup per chunk: nobody
    ever waits -- no helper at all, where every group inside the batch is complete from its owners alone"""
    b = _batch(n_chunks, last)
    _run(harness, b, grid, harness.cp_default_patience())
    got, exp_sums = _groups(harness, b)
    assert [g for g in got[:len(exp_sums)]] == [(64, s) for s in exp_sums]
    assert all(count <= 64 for count, _ in got)
    if n_chunks % 64:                                              # the partial group at the end: as many owners as it has chunks
        assert got[-1] == (n_chunks % 64, int(b["chunk_totals"][64 * (n_chunks // 64):].sum()))


def test_a_missing_total_is_waited_for_not_taken_as_zero(harness):
    """grid 3 over 5 chunks: workgroup 0's second chunk (3) needs the totals of chunks 1 and 2, whose owners run later -- the result is right
    only if it computes them itself, and their words then hold the helper's value, which the owner's own store repeats"""
    b = _batch(5, 1024)
    _run(harness, b, 3, 8)
    for c in (1, 2, 4):
        assert harness.cp_state_word(c) == (1 << 62) | int(b["chunk_totals"][c])


def test_more_than_64_whole_groups(harness):
    """a range of predecessors wider than 4,096 chunks takes a second round of group words, read fresh: 4,200 chunks, a workgroup per
    chunk (grid 4,300), so the last workgroups sum 65 whole groups and a partial one.  (Plain words only -- one token or none -- and the
    expectation by cumsum: the point is the arithmetic over the groups, and 4.3 M pre-tokens through the loop of _batch take a minute.)"""
    n_chunks, chunk = 4200, 1024
    P = n_chunks * chunk - 1000
    rng = np.random.default_rng(7)
    ids = rng.integers(0, 1 << 20, P).astype(np.uint32)
    none = rng.integers(0, 100, P) < 3 + (np.arange(P) // chunk) % 5      # a share of empty pre-tokens that differs from chunk to chunk
    tok0 = np.where(none, 0, TOK_ONE | ids).astype(np.uint32)
    cnt = (~none).astype(np.int64)
    tok_start = np.concatenate([[0], np.cumsum(cnt)])
    doc_pt = np.array(sorted(rng.integers(0, P, 5000).tolist() + [0, 64 * chunk, 64 * chunk, P, P]), dtype=np.uint32)
    b = dict(P=P, tok0=tok0, rows=np.zeros((1, 4), dtype=np.uint32), tmp=np.zeros(1, dtype=np.uint32), doc_pt=doc_pt, ids=ids[~none], tok_start=tok_start,
             tok_offsets=tok_start[doc_pt.astype(np.int64)], chunk_totals=np.add.reduceat(cnt, np.arange(0, P, chunk)))
    _run(harness, b, 4300, 8, want_pt_tokoff=False)
    got, exp_sums = _groups(harness, b)
    assert len(exp_sums) == 65 and got[:65] == [(64, s) for s in exp_sums] and got[65][0] == n_chunks - 65 * 64
