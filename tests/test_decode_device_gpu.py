"""-m gpu: the device entry of decode_batch (tkamd_decode_batch_device) -- ids in HBM as ranges over any array, valid UTF-8 text left in
HBM -- against the decode oracle for every decoder case of tests/decode_cases.py, the range gather at its edges, the lossy UTF-8
repair where an id sequence cuts a character, and decode -> encode with two tokenizers without a host copy in between.
The raw-pointer tests run under the SIMT emulation as well ("device" memory is numpy memory there); the torch ones are needs_hw."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from oracle.decode_oracle import DecodeOracle, bytes_char
from tests import decode_cases as dc
from tests.helpers import load_tokenizer_json

pytestmark = pytest.mark.gpu

PAD = 64                                                   # TKAMD_TEXT_PAD


def _on_emulation() -> bool:
    if os.environ.get("TKAMD_SIMT") != "1":
        return False
    import torch
    return not torch.cuda.is_available()


def _up(a: np.ndarray):
    """(what keeps the memory alive, device pointer) of a numpy array"""
    a = np.ascontiguousarray(a)
    if _on_emulation():
        return a, a.ctypes.data
    import torch
    t = torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()
    return t, t.data_ptr()


def _down(text):
    """(the text with its PAD bytes of slack, doc offsets, the byte count as the device holds it) of a DeviceText"""
    raw, off = text.to_host(slack=PAD)
    return raw.tobytes(), [int(x) for x in off], text.n_bytes_device()


def _decode(tk, ids, begin, end, skip, dtype="uint32"):
    """One tkamd_decode_batch_device call over host arrays put on the device -> the byte string of every sequence, with the contract of
    the result checked on the way: a monotone CSR that ends at n_bytes, the count on the device, the zero slack, valid UTF-8."""
    ids = np.asarray(ids, dtype={"uint32": np.uint32, "int32": np.int32, "int64": np.int64}[dtype])
    begin, end = np.asarray(begin, dtype=np.int64), np.asarray(end, dtype=np.int64)
    keep = [_up(ids), _up(begin), _up(end)]
    text = tk.decode_batch_device(keep[0][1], len(ids), keep[1][1], keep[2][1], len(begin), skip_special_tokens=skip, ids_dtype=dtype)
    raw, off, n_dev = _down(text)
    assert text.n_docs == len(begin) and len(off) == len(begin) + 1
    assert off[0] == 0 and off[-1] == text.n_bytes == n_dev, (off[:3], off[-1], text.n_bytes, n_dev)
    assert all(a <= b for a, b in zip(off[:-1], off[1:]))
    assert raw[text.n_bytes:] == b"\0" * PAD
    out = [raw[a:b] for a, b in zip(off[:-1], off[1:])]
    for s in out:
        s.decode("utf-8")                                      # strict: every sequence on its own is valid UTF-8
    assert text.to_strings() == [s.decode("utf-8") for s in out]
    return out


def _csr(seqs):
    off = np.zeros(len(seqs) + 1, dtype=np.int64)
    np.cumsum([len(q) for q in seqs], out=off[1:])
    return [i for q in seqs for i in q], off[:-1], off[1:]


def _diff(label, got, exp):
    assert len(got) == len(exp), (label, len(got), len(exp))
    bad = [(i, got[i][:80], exp[i][:80]) for i in range(len(exp)) if got[i] != exp[i]]
    assert not bad, f"{label}: {len(bad)} of {len(exp)} sequences differ, first {bad[0]!r}"


def _lossy(b: bytes) -> bytes:
    return b.decode("utf-8", "replace").encode("utf-8")


@pytest.mark.parametrize("k", range(len(dc.DECODERS)), ids=dc.case_id)
def test_decode_batch_device_vs_oracle(k):
    """Every decoder case as a packed CSR, both skip values: the bytes are the oracle's (behind from_utf8_lossy for the ByteLevel
    decoder), the strings are Tokenizer.decode_batch's.  Token counts 0, 1, 255, 256, 257 and 8193 among them."""
    import tokenizers_amd as ta
    case = dc.Case(k)
    tk = ta.Tokenizer.from_str(case.json, device=0)
    o = DecodeOracle(case.json)
    byte_level = (case.decoder or {}).get("type") == "ByteLevel"
    batches = dc.sequences(case, dc.rng_for(k))
    flat = [i for q in next(b for b in batches if b.name == "tokens-8193").seqs for i in q]
    for n in (0, 1, 255, 256, 257, 8193):
        batches.append(dc.Batch(f"count-{n}", [flat[:n // 3], flat[n // 3:n]]))
    for b in batches:
        ids, begin, end = _csr(b.seqs)
        for skip in (True, False):
            label = f"{b.name} skip={skip}"
            exp = [o.decode_bytes(q, skip) for q in b.seqs]
            if byte_level:
                exp = [_lossy(x) for x in exp]
            got = _decode(tk, ids, begin, end, skip)
            _diff(label, got, exp)
            _diff(label + " (strings)", [x.decode("utf-8") for x in got], tk.decode_batch(b.seqs, skip_special_tokens=skip))


def _byte_level_case():
    k = next(i for i, (name, dec) in enumerate(dc.DECODERS) if name == "gpt2_added_tokens" and dec == dc.OWN)
    return k, dc.Case(k)


def test_ranges_in_any_order_with_gaps_overlaps_and_nothing():
    import tokenizers_amd as ta
    k, case = _byte_level_case()
    tk, o = ta.Tokenizer.from_str(case.json, device=0), DecodeOracle(case.json)
    rng = dc.rng_for(100 + k)
    seqs = [dc._mixed_seq(case, rng, int(n)) for n in [0, 1, 7, 300, 31, 32, 33, 0, 257, 5]]
    ids, begin, end = _csr(seqs)
    begin, end = begin.copy(), end.copy()
    exp = lambda bs, es, skip, src=None: [_lossy(o.decode_bytes((src or ids)[a:b], skip)) for a, b in zip(bs, es)]
    for skip in (True, False):
        # reversed
        _diff("reversed", _decode(tk, ids, begin[::-1], end[::-1], skip), exp(begin[::-1], end[::-1], skip))
        # gaps: every range loses its first and its last id (what is shorter than two becomes empty), and a whole sequence is left out
        gb = np.minimum(begin + 1, end)
        ge = np.maximum(end - 1, gb)
        keep = [d for d in range(len(seqs)) if d != 3]
        _diff("gaps", _decode(tk, ids, gb[keep], ge[keep], skip), exp(gb[keep], ge[keep], skip))
        # the same range named twice, ranges that overlap, one range over everything, empty ranges in every place
        ob = [begin[3], begin[3], begin[3] + 10, 0, 0, len(ids), 5, begin[8], begin[3]]
        oe = [end[3], end[3], end[4] + 3, len(ids), 0, len(ids), 5, end[8], end[3]]
        _diff("overlaps", _decode(tk, ids, ob, oe, skip), exp(ob, oe, skip))
        # no sequence at all, over ids and over nothing
        assert _decode(tk, ids, [], [], skip) == [] and _decode(tk, [], [], [], skip) == []
        assert _decode(tk, [], [0, 0], [0, 0], skip) == [b"", b""]
        # int32 bit patterns are the uint32 ids
        _diff("int32", _decode(tk, ids, begin, end, skip, dtype="int32"), exp(begin, end, skip))
        # int64 with values that are no uint32 between real ids: they decode to nothing, as an id beyond the vocabulary does
        junk = [-100, -1, 2 ** 32, 2 ** 40, -2 ** 63, 2 ** 63 - 1]
        wide, wb, we, clean, clean_b, clean_e = [], [], [], [], [], []
        for d, q in enumerate(seqs):
            wb.append(len(wide))
            clean_b.append(len(clean))
            for j, i in enumerate(q):
                if (j + d) % 3 == 0:
                    wide.append(junk[(j + d) % len(junk)])
                wide.append(i)
                clean.append(i)
            wide.append(junk[d % len(junk)])
            we.append(len(wide))
            clean_e.append(len(clean))
        _diff("int64", _decode(tk, wide, wb, we, skip, dtype="int64"), exp(clean_b, clean_e, skip, clean))
        _diff("int64 ids beyond the vocabulary", _decode(tk, [case.n_ids + 5, 2 ** 32 - 1, 2 ** 31], [0], [3], skip, dtype="int64"), [b""])


def test_bad_ranges_are_refused_on_the_device_and_leave_the_handle_sound():
    import tokenizers_amd as ta
    k, case = _byte_level_case()
    tk, o = ta.Tokenizer.from_str(case.json, device=0), DecodeOracle(case.json)
    rng = dc.rng_for(200 + k)
    seqs = [dc._mixed_seq(case, rng, int(n)) for n in [12, 40, 3, 300]]
    ids, begin, end = _csr(seqs)
    good = [_lossy(o.decode_bytes(q, True)) for q in seqs]
    _diff("before", _decode(tk, ids, begin, end, True), good)
    n = len(ids)
    for bb, ee, who in (([0, 30, 5, 60], [12, 20, 9, 61], "sequence 1: begin > end"),
                        ([0, 12, 52, 55], [12, 52, 55, n + 1], "sequence 3: end > n_ids"),
                        ([0, -1, 52, 70], [12, 52, n + 7, 60], "sequence 1: begin < 0"),          # the FIRST bad one is named
                        ([n + 1], [n + 1], "sequence 0: end > n_ids")):
        with pytest.raises(ValueError, match=who):
            _decode(tk, ids, bb, ee, True)
        _diff("after " + who, _decode(tk, ids, begin, end, True), good)
    # the limit of 2^31 tokens holds for the SUM of the ranges, which may overlap: many sequences naming one small range pass 2^31, pass
    # 2^32 (a 32-bit sum would come out as 2^30 and as exactly 0) -- refused before anything is sized or gathered
    small = np.zeros(1 << 20, dtype=np.uint32)
    for n_seqs in (2048, 3072, 4096, 5120, 1 << 16):
        with pytest.raises(ValueError, match="more than 2\\^31 tokens"):
            _decode(tk, small, np.zeros(n_seqs, dtype=np.int64), np.full(n_seqs, 1 << 20, dtype=np.int64), True)
        _diff(f"after {n_seqs} x 2^20 tokens", _decode(tk, ids, begin, end, True), good)
    _decode(tk, small[:256], np.zeros(300, dtype=np.int64), np.full(300, 256, dtype=np.int64), True)      # (many overlapping ranges under the limit are fine)
    # one range of 2^31 ids or more is refused by itself (the check comes before any read: the array need not exist)
    keep = [_up(small), _up(np.array([0, 5], dtype=np.int64)), _up(np.array([4, 5 + (1 << 31)], dtype=np.int64))]
    with pytest.raises(ValueError, match="sequence 1: 2\\^31 ids or more"):
        tk.decode_batch_device(keep[0][1], 1 << 40, keep[1][1], keep[2][1], 2)
    _diff("after a range of 2^31 ids", _decode(tk, ids, begin, end, True), good)
    with pytest.raises(ValueError, match="ids_dtype"):
        tk.decode_batch_device(0, 0, 0, 0, 0, ids_dtype="int16")


def test_lossy_repair_where_the_ids_cut_a_character():
    """ByteLevel: one token per byte, so a sequence is any byte string.  An invalid subpart at the start, at the end, as the only content,
    split over two sequences (each gets a U+FFFD of its own), and behind as much ASCII as puts it across a lane (16 bytes), a
    workgroup of the length pass (256) and a workgroup of the counting pass (4096)."""
    import tokenizers_amd as ta
    k, case = _byte_level_case()
    tk = ta.Tokenizer.from_str(case.json, device=0)
    vocab = json.loads(case.json)["model"]["vocab"]
    b2c = bytes_char()
    tok = lambda raw: [vocab[b2c[b]] for b in raw]
    euro, smile = "€".encode(), "\U0001f600".encode()          # E2 82 AC, F0 9F 98 80
    docs = [b"\xacab", b"ab\xe2\x82", b"\xe2\x82", b"\xac", b"\xe2\x82", b"\xac", b"\xff", b"", euro, b"a" + euro[:2], euro[2:] + b"b",
            smile[:3], smile[3:], smile[:1], smile[1:], b"\xe0\x80\x80", b"\xed\xa0\x80", b"\xf4\x90\x80\x80", b"\xc0\xaf", b"\xef\xbf\xbd"]
    for n in (13, 14, 15, 16, 17, 255, 256, 257, 4093, 4094, 4095, 4096, 4097):
        a = b"a" * n
        docs += [a + euro[:2], euro[2:] + b"z", a + euro, a + euro[:2] + b"a", a + euro[:1], euro[1:], a + smile[:2], smile[2:]]
    ids, begin, end = _csr([tok(d) for d in docs])
    exp = [_lossy(d) for d in docs]
    assert exp[1] == b"ab\xef\xbf\xbd" and exp[2] == exp[3] == b"\xef\xbf\xbd"
    _diff("repair", _decode(tk, ids, begin, end, True), exp)
    _diff("repair reversed", _decode(tk, ids, begin[::-1], end[::-1], True), exp[::-1])
    # a text with nothing to repair keeps its buffer; then a large one that needs it, then a small one again on the same handle
    _diff("clean", _decode(tk, tok(b"plain text" + euro), [0, 10], [10, 13], True), [b"plain text", euro])
    big = [docs[int(j)] for j in dc.rng_for(300).integers(0, len(docs), size=400)]
    bi, bb, be = _csr([tok(d) for d in big])
    _diff("large", _decode(tk, bi, bb, be, True), [_lossy(d) for d in big])
    _diff("small after large", _decode(tk, tok(b"a\xe2\x82"), [0, 1], [1, 3], True), [b"a", b"\xef\xbf\xbd"])
    _diff("clean after large", _decode(tk, tok(b"ok"), [0], [2], True), [b"ok"])


@pytest.mark.needs_hw
def test_decode_tensor_then_encode_with_another_tokenizer_without_a_host_copy():
    """A's ids in a padded [64, L] int64 tensor -> A.decode_tensor -> B.encode_batch_device over the text where it lies, on one stream:
    the ids are what the host path gives, B.encode_batch_fast(A.decode_batch(...)).  One document's ids are cut inside a character, so
    B reads repaired text."""
    import torch
    import tokenizers_amd as ta
    from oracle import synth
    A = ta.Tokenizer.from_str(load_tokenizer_json("gpt2_synth_50257"), device=0)
    B = ta.Tokenizer.from_str(load_tokenizer_json("llama3_small_6000"), device=0)
    docs = synth.gen_lines(63, text_seed=41)[:63] + ["café € 中文 \U0001f600"]
    buf, off = ta.pack_documents(docs)
    st = torch.cuda.current_stream().cuda_stream
    d_text, d_off = torch.from_numpy(np.array(buf)).cuda(), torch.from_numpy(np.array(off)).cuda()
    enc = A.encode_batch_device(d_text.data_ptr(), d_off.data_ptr(), len(docs), int(off[-1]), stream=st).sync()
    flat, tok_off = enc.ids_tensor().to(torch.int64), enc.tok_offsets_tensor().clone()
    lens = (tok_off[1:] - tok_off[:-1]).clone()
    host_ids = [flat[int(a):int(b)].tolist() for a, b in zip(tok_off[:-1].tolist(), tok_off[1:].tolist())]
    cut = next(n for n in range(len(host_ids[-1]) - 1, 0, -1) if "�" in A.decode_batch([host_ids[-1][:n]])[0])
    host_ids[-1] = host_ids[-1][:cut]
    lens[-1] = cut
    L = int(lens.max()) + 3
    right = torch.full((len(docs), L), -100, dtype=torch.int64, device="cuda")
    left = torch.full((len(docs), L), -100, dtype=torch.int64, device="cuda")
    for r, q in enumerate(host_ids):
        right[r, :len(q)] = torch.tensor(q, device="cuda")
        left[r, L - len(q):] = torch.tensor(q, device="cuda")
    want_text = A.decode_batch(host_ids)
    assert "�" in want_text[-1]
    want = B.encode_batch_fast(want_text, add_special_tokens=False)
    for ids2d, kw in ((right, dict(lengths=lens)), (left, dict(lengths=lens, starts=L - lens)), (right.to(torch.int32), dict(lengths=lens.tolist()))):
        text = A.decode_tensor(ids2d, **kw)
        got = B.encode_batch_device(text.bytes_ptr, text.doc_offsets_ptr, text.n_docs, text.n_bytes, stream=st, unsynced=True).sync()
        assert got.tok_offsets_tensor().cpu().tolist() == [int(x) for x in want.tok_offsets]
        assert np.array_equal(got.ids_tensor().cpu().numpy().view(np.uint32), want.ids)
        assert text.to_strings() == want_text                   # (after the encode: it has not moved the text)
        raw, doff = text.to_host()
        assert text.bytes_tensor().cpu().numpy().tobytes() == raw.tobytes() and text.doc_offsets_tensor().cpu().tolist() == doff.tolist()
    # whole rows (no lengths: the -100 fillers decode to nothing) and a 1-D tensor with lengths
    assert A.decode_tensor(right).to_strings() == want_text
    assert A.decode_tensor(torch.cat([torch.tensor(q, dtype=torch.int64, device="cuda") for q in host_ids]), lengths=lens).to_strings() == want_text
    with pytest.raises(ValueError):
        A.decode_tensor(flat)
    with pytest.raises(TypeError):
        A.decode_tensor(right.to(torch.float32))
