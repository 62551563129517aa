"""-m gpu: the dense entry (tkamd_encode_batch_device_dense / Tokenizer.encode_batch_device_dense / Tokenizer.encode_tensor) -- text in
HBM in, padded [n_rows, width] int64 / int32 arrays in the caller's memory out -- against the reference wheel's recorded answers
(tests/golden/dense_vectors.json.gz, tools/make_golden_dense.py) for every case and shape of tests/dense_cases.py, and against the same
handle's own encode_batch views (cheap; catches the two paths drifting apart; not the oracle).  The raw-pointer tests run under the SIMT
emulation as well ("device" memory is numpy memory there); the torch ones are needs_hw."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

from tests import dense_cases as dn
from tests.helpers import load_tokenizer_json, load_vectors

pytestmark = pytest.mark.gpu

FILL = -77                                                  # what the outputs hold before a call: no element may keep it
NP = {"int64": np.int64, "int32": np.int32}


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
    t = torch.from_numpy(a).cuda()
    return t, t.data_ptr()


def _host(keep) -> np.ndarray:
    return keep if isinstance(keep, np.ndarray) else keep.cpu().numpy()


@pytest.fixture(scope="module")
def vectors():
    return load_vectors("dense")["cases"]


_handles = {}


def _tokenizer(case):
    import tokenizers_amd as ta
    key = case["name"]
    if key not in _handles:
        _handles.clear()                                     # (one handle at a time: a case's tests come together)
        _handles[key] = ta.Tokenizer.from_str(dn.tokenizer_json(case), device=0)
    return _handles[key]


def _flat(inputs):
    return [s for it in inputs for s in it] if inputs and isinstance(inputs[0], tuple) else list(inputs)


def _dense(tk, case, inputs, dtype="int64", fields=dn.FIELDS, sync=True, offset_elems=0):
    """One encode_batch_device_dense call over host inputs put on the device -> {field: [n_rows, width(, 2)] numpy array}.  Every
    output starts out as FILL; offset_elems shifts every output by that many elements off its allocation's start (alignment)."""
    import tokenizers_amd as ta
    docs = _flat(inputs)
    buf, off = ta.pack_documents(docs)
    text, offs = _up(np.array(buf)), _up(np.array(off))
    n_rows, width = len(inputs), case["width"]
    outs, ptrs = {}, {}
    for k in fields:
        shape = (n_rows, width, 2) if k == "offset_mapping" else (n_rows, width)
        n = int(np.prod(shape))
        outs[k] = (_up(np.full(n + offset_elems + 1, FILL, dtype=NP[dtype])), shape)
        ptrs[k] = outs[k][0][1] + offset_elems * np.dtype(NP[dtype]).itemsize
    b = tk.encode_batch_device_dense(text[1], offs[1], len(docs), int(off[-1]), ptrs, width, dtype=dtype, pairs=case["pairs"],
                                     add_special_tokens=case["add_special_tokens"], offsets="char" if "offset_mapping" in fields else "none",
                                     word_ids="word_ids" in fields)
    if sync:
        b.sync()
    got = {}
    for k, ((keep, _), shape) in outs.items():
        h = _host(keep)
        n = int(np.prod(shape))
        assert (h[:offset_elems] == FILL).all() and h[offset_elems + n] == FILL, f"{k}: written outside the array"
        got[k] = h[offset_elems:offset_elems + n].reshape(shape)
    return got, b


def _expect(vec, n=None):
    """the recorded answer's first n rows (all of them: None), per field"""
    return {k: np.asarray(vec[k][:n], dtype=np.int64) for k in dn.FIELDS}


def _shaped(exp, k, n_rows, width):
    return exp[k].reshape((n_rows, width, 2) if k == "offset_mapping" else (n_rows, width))


def _own(tk, case, inputs):
    """the same handle's encode_batch views, stacked"""
    be = tk.encode_batch(list(inputs), add_special_tokens=case["add_special_tokens"])
    encs = [be[i] for i in range(len(be))]
    return {"input_ids": [e.ids for e in encs], "attention_mask": [e.attention_mask for e in encs], "token_type_ids": [e.type_ids for e in encs],
            "special_tokens_mask": [e.special_tokens_mask for e in encs], "offset_mapping": [[list(o) for o in e.offsets] for e in encs],
            "word_ids": [[-1 if w is None else w for w in e.word_ids] for e in encs]}


def _check(label, got, exp, n_rows, width, fields=dn.FIELDS):
    for k in fields:
        want = _shaped(exp, k, n_rows, width)
        assert got[k].shape == want.shape, (label, k, got[k].shape, want.shape)
        if not np.array_equal(got[k].astype(np.int64), want):
            r = int(np.argwhere(got[k].astype(np.int64) != want)[0][0])
            raise AssertionError(f"{label}: {k} differs in row {r}: got {got[k][r].tolist()}, expected {want[r].tolist()}")


@pytest.mark.parametrize("dtype", ["int64", "int32"])
@pytest.mark.parametrize("name", dn.SHAPE_CASES)
def test_every_width_and_row_count_vs_the_wheel(name, dtype, vectors):
    """width in {1 .. 65} x n_rows in {0, 1, 2, 3, 255, 256, 257}: the first n rows of the wheel's answer for the 257 documents (Fixed
    padding: every encoding stands on its own).  257 x 65 elements pass one workgroup's share (512 int64 / 1024 int32 elements) and, on
    the emulation's 8 workgroups, the grid's."""
    case = dn.BY_NAME[name]
    tk = _tokenizer(case)
    assert tk.dense_width(case["add_special_tokens"]) == case["width"]
    for n in dn.ROWS:
        got, b = _dense(tk, case, case["inputs"][:n], dtype)
        _check(f"{name} n_rows={n} {dtype}", got, _expect(vectors[name], n), n, case["width"])
        assert b._capacity == n * case["width"]
    own = {k: np.asarray(v, dtype=np.int64) for k, v in _own(tk, case, case["inputs"][:3]).items()}
    _check(f"{name} own views", _dense(tk, case, case["inputs"][:3], dtype)[0], own, 3, case["width"])


FEATURE_CASES = [c["name"] for c in dn.CASES if c["name"] not in dn.SHAPE_CASES and c["name"] not in dn.DIGEST_ONLY]


@pytest.mark.parametrize("name", FEATURE_CASES)
def test_every_layout_vs_the_wheel_alone_and_first_in_a_batch(name, vectors):
    """Padding side, pad_to_multiple_of, truncation from the left, a row without padding, empty documents, pairs under every strategy
    (BERT type ids, a RoBERTa template), a typed single template, prefix-only templates, no special tokens: the whole batch and its
    first input alone, int64 and int32, against the wheel and against the handle's own encode_batch."""
    case = dn.BY_NAME[name]
    tk = _tokenizer(case)
    n, width = len(case["inputs"]), case["width"]
    assert tk.dense_width(case["add_special_tokens"], case["pairs"]) == width
    own = {k: np.asarray(v, dtype=np.int64) for k, v in _own(tk, case, case["inputs"]).items()}
    for dtype in ("int64", "int32"):
        _check(f"{name} {dtype}", _dense(tk, case, case["inputs"], dtype)[0], _expect(vectors[name]), n, width)
        _check(f"{name} alone {dtype}", _dense(tk, case, case["inputs"][:1], dtype)[0], _expect(vectors[name], 1), 1, width)
    _check(f"{name} own views", _dense(tk, case, case["inputs"])[0], own, n, width)


@pytest.mark.parametrize("name", ["pairs_bert_longest_left", "typed_single", "prefix_only_spm"])
def test_every_optional_output_null_in_turn_and_unaligned_arrays(name, vectors):
    """Each optional array left out in turn (the others are what they were), only input_ids, and every array one element off a 16-byte
    boundary (the element-wise stores)."""
    case = dn.BY_NAME[name]
    tk = _tokenizer(case)
    n, width = len(case["inputs"]), case["width"]
    exp = _expect(vectors[name])
    for drop in dn.FIELDS[1:]:
        fields = tuple(k for k in dn.FIELDS if k != drop)
        _check(f"{name} without {drop}", _dense(tk, case, case["inputs"], fields=fields)[0], exp, n, width, fields)
    _check(f"{name} input_ids only", _dense(tk, case, case["inputs"], fields=("input_ids",))[0], exp, n, width, ("input_ids",))
    for dtype in ("int64", "int32"):
        _check(f"{name} unaligned {dtype}", _dense(tk, case, case["inputs"], dtype, offset_elems=1)[0], exp, n, width)


@pytest.mark.needs_hw
def test_rows_beyond_one_grid_of_workgroups(vectors):
    """8200 x 128 elements: more than 2048 workgroups x 256 lanes x 2 int64 elements, so the grid-stride loop turns; by digest."""
    case = dn.BY_NAME["shape_grid"]
    tk = _tokenizer(case)
    got, _ = _dense(tk, case, case["inputs"])
    h = hashlib.sha256()
    for k in dn.FIELDS:
        h.update(np.ascontiguousarray(got[k], dtype="<i8").tobytes())
    assert len(case["inputs"]) == vectors["shape_grid"]["n_rows"] and h.hexdigest() == vectors["shape_grid"]["digest"]


def _raw(tk, n_docs, flags, dst, text_ptr, off_ptr, n_bytes):
    from tokenizers_amd import _lib
    res = _lib.DeviceResult()
    _lib.check(tk._lib.tkamd_encode_batch_device_dense(tk._h, text_ptr, off_ptr, n_docs, n_bytes, flags, 0, C.byref(dst), C.byref(res)))
    return res


def test_refusals_name_the_missing_piece_and_leave_the_handle_sound(vectors):
    import tokenizers_amd as ta
    from tokenizers_amd import _lib
    case = dn.BY_NAME["pairs_bert_longest"]
    single = dict(case, inputs=[a for a, _ in case["inputs"]], pairs=False)
    tk = _tokenizer(case)
    docs = _flat(case["inputs"])
    buf, off = ta.pack_documents(docs)
    text, offs = _up(np.array(buf)), _up(np.array(off))
    n_rows, width = len(case["inputs"]), case["width"]
    arr = _up(np.full(n_rows * width * 2 + 8, FILL, dtype=np.int64))
    nb = int(off[-1])

    def dst(**kw):
        d = dict(input_ids=arr[1], attention_mask=None, token_type_ids=None, special_tokens_mask=None, offsets=None, word_ids=None, n_rows=n_rows,
                 width=width, dtype_flags=0)
        d.update(kw)
        return _lib.DenseOut(*[d[f] for f, _ in _lib.DenseOut._fields_])

    pairs = _lib.PAIRS | _lib.ADD_SPECIAL
    for flags, d, n_docs, msg in (
            (pairs | _lib.WANT_OVERFLOW, dst(), len(docs), "TKAMD_WANT_OVERFLOW: the number of rows"),
            (pairs, dst(offsets=arr[1]), len(docs), "offsets asked for without an offsets mode"),
            (pairs, dst(word_ids=arr[1]), len(docs), "word_ids asked for without TKAMD_WANT_WORD_IDS"),
            (pairs, dst(n_rows=n_rows + 1), len(docs), f"n_rows is {n_rows + 1}, the batch has {n_rows} pairs"),
            (_lib.ADD_SPECIAL, dst(), len(docs), f"n_rows is {n_rows}, the batch has {2 * n_rows} documents"),
            (pairs, dst(width=width + 1), len(docs), f"width is {width + 1}, tkamd_dense_width says {width}"),
            (pairs, dst(input_ids=None), len(docs), "input_ids is null"),
            (pairs, dst(dtype_flags=2), len(docs), "unknown dtype_flags")):
        with pytest.raises(ValueError, match=msg):
            _raw(tk, n_docs, flags, d, text[1], offs[1], nb)
        assert (_host(arr[0]) == FILL).all(), msg             # refused in front of all device work
        _check("after " + msg, _dense(tk, case, case["inputs"])[0], _expect(vectors[case["name"]]), n_rows, width)
    # the flag belongs to the dense entry alone: the other entries refuse it, pre-tokenized input included
    res = _lib.DeviceResult()
    for call in (lambda: tk._lib.tkamd_encode_batch_device(tk._h, text[1], offs[1], len(docs), nb, _lib.WANT_DENSE, 0, C.byref(res)),
                 lambda: tk._lib.tkamd_encode_batch_words_device(tk._h, text[1], offs[1], len(docs), nb, offs[1], 0, _lib.WANT_DENSE, 0, C.byref(res))):
        with pytest.raises(ValueError, match="only tkamd_encode_batch_device_dense takes this flag"):
            _lib.check(call())
    b = C.c_void_p()
    with pytest.raises(ValueError, match="only tkamd_encode_batch_device_dense takes this flag"):
        _lib.check(tk._lib.tkamd_encode_batch(tk._h, buf.ctypes.data, off.ctypes.data, len(docs), _lib.WANT_DENSE, C.byref(b)))
    _check("after the other entries", _dense(tk, case, case["inputs"])[0], _expect(vectors[case["name"]]), n_rows, width)
    # the width's conditions, each by what is missing
    d = json.loads(dn.tokenizer_json(case))
    for edit, msg in ((lambda x: x.pop("truncation"), "needs a `truncation` section"),
                      (lambda x: x.pop("padding"), "needs a `padding` section"),
                      (lambda x: x["padding"].update(strategy="BatchLongest"), "needs Fixed padding"),
                      (lambda x: x["truncation"].update(max_length=width + 1), f"max_length {width + 1} exceeds the padded width {width}"),
                      (lambda x: x["truncation"].update(max_length=2), "max_length 2 is below the 3 special tokens")):
        x = json.loads(json.dumps(d))
        edit(x)
        bad = ta.Tokenizer.from_str(json.dumps(x), device=0)
        with pytest.raises(ValueError, match=msg):
            bad.dense_width(True, pairs=True)
        with pytest.raises(ValueError, match=msg):
            _raw(bad, len(docs), pairs, dst(), text[1], offs[1], nb)
        # ... and the handle still encodes
        assert len(bad.encode_batch_fast([a for a, _ in case["inputs"]])) == n_rows
    # max_length 2 holds a single sequence's two special tokens: a width again
    x = json.loads(json.dumps(d))
    x["truncation"].update(max_length=2)
    assert ta.Tokenizer.from_str(json.dumps(x), device=0).dense_width(True) == width
    del single


def test_a_multi_device_handle_is_refused(vectors):
    import tokenizers_amd as ta
    case = dn.BY_NAME["left_padding"]
    tk = ta.Tokenizer.from_str(dn.tokenizer_json(case), device=[0, 0])
    with pytest.raises(ValueError, match="dense output on a multi-device handle"):
        _dense(tk, case, case["inputs"])
    assert len(tk.encode_batch_fast(list(case["inputs"]))) == len(case["inputs"])


def test_dense_then_plain_then_dense_on_one_handle_and_stream(vectors):
    """A dense call, a plain encode_batch_device call and the dense call again: equal arrays, and the plain call's CSR is the padded
    rows the dense call's `out` names."""
    import tokenizers_amd as ta
    case = dn.BY_NAME["typed_single_left"]
    tk = _tokenizer(case)
    n, width = len(case["inputs"]), case["width"]
    first, b1 = _dense(tk, case, case["inputs"])
    buf, off = ta.pack_documents(list(case["inputs"]))
    text, offs = _up(np.array(buf)), _up(np.array(off))
    plain = tk.encode_batch_device(text[1], offs[1], n, int(off[-1]), unsynced=True).sync()
    assert plain.n_tokens == n * width and b1.n_tokens == n * width
    second, _ = _dense(tk, case, case["inputs"])
    _check("first", first, _expect(vectors[case["name"]]), n, width)
    for k in dn.FIELDS:
        assert np.array_equal(first[k], second[k]), k


MANY = [" ".join("q%dz%dx" % (i, 7 * i + j) for j in range(12)) for i in range(40)]      # (tests/test_launch_sequence.py: overflows a tiny queue once)


def test_a_queue_overflow_is_repaired_by_sync_into_the_callers_arrays():
    """TKAMD_Q16_DIV (test hook, read when the handle is made): the <= 16-byte queue overflows, sync() grows it and runs the batch
    again from the workspace's flags and destination -- the caller's arrays then hold the rows of a handle whose queue never overflowed.
    (Ids and masks: the offsets pass of a batch whose queue overflowed is not this stage's to exercise.)"""
    import tokenizers_amd as ta
    fields = ("input_ids", "attention_mask", "token_type_ids", "special_tokens_mask")
    case = dict(dn.BY_NAME["bytelevel_plain"], inputs=MANY)
    js = dn.tokenizer_json(case)
    want, _ = _dense(ta.Tokenizer.from_str(js, device=0), case, MANY, fields=fields)
    saved = {k: os.environ.get(k) for k in ("TKAMD_TEST_HOOKS", "TKAMD_Q16_DIV")}
    os.environ.update(TKAMD_TEST_HOOKS="1", TKAMD_Q16_DIV="100000")
    try:
        tiny = ta.Tokenizer.from_str(js, device=0)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    got, _ = _dense(tiny, case, MANY, fields=fields)        # (syncs)
    assert tiny.queue_sizes()["q16_div"] == 2, "the queue did not overflow exactly once"
    for k in fields:
        assert np.array_equal(got[k], want[k]), k
    own = {k: np.asarray(v, dtype=np.int64) for k, v in _own(tiny, case, MANY).items()}
    _check("own views", got, own, len(MANY), case["width"], fields)
    assert (got["attention_mask"].sum(axis=1) > 4).all()    # (real rows, not padding alone)


def test_live_differential_against_the_wheel(ref_tokenizers):
    """300 seeded strings of the fuzz alphabet through the wheel and through the dense entry, single sequences and pairs."""
    import random
    from tests import fuzz_cases as fz
    rnd = random.Random(20240607)
    texts = [fz._text(rnd, fz.MAX_CHARS) for _ in range(300)]
    for name, inputs in (("left_padding", texts), ("pairs_bert_longest_left", list(zip(texts[::2], texts[1::2]))), ("prefix_only_llama3", texts),
                         ("unigram_left", texts)):
        case = dict(dn.BY_NAME[name], inputs=inputs)
        js = dn.tokenizer_json(case)
        encs = ref_tokenizers.Tokenizer.from_str(js).encode_batch(list(inputs), add_special_tokens=case["add_special_tokens"])
        exp = {"input_ids": [e.ids for e in encs], "attention_mask": [e.attention_mask for e in encs], "token_type_ids": [e.type_ids for e in encs],
               "special_tokens_mask": [e.special_tokens_mask for e in encs], "offset_mapping": [[list(o) for o in e.offsets] for e in encs],
               "word_ids": [[-1 if w is None else w for w in e.word_ids] for e in encs]}
        got, _ = _dense(_tokenizer(case), case, inputs)
        _check(f"live {name}", got, {k: np.asarray(v, dtype=np.int64) for k, v in exp.items()}, len(inputs), case["width"])


# ---- encode_tensor: torch tensors on the device (needs_hw) ----
def _tensors_equal(tb, exp, n_rows, width, keys):
    for k in keys:
        want = _shaped(exp, k, n_rows, width)
        assert np.array_equal(tb[k].cpu().numpy().astype(np.int64), want), k


@pytest.mark.needs_hw
def test_encode_tensor_from_strings_pairs_device_text_and_a_tensor_pair(vectors):
    import torch
    import tokenizers_amd as ta
    keys = dn.FIELDS
    kw = dict(return_special_tokens_mask=True, return_offsets_mapping=True, return_word_ids=True)
    # list[str], both dtypes: a torch op on the same stream right behind the call, no sync() in between
    case = dn.BY_NAME["left_padding"]
    tk = _tokenizer(case)
    n, width = len(case["inputs"]), case["width"]
    exp = _expect(vectors[case["name"]])
    for dtype in (torch.int64, torch.int32):
        tb = tk.encode_tensor(list(case["inputs"]), dtype=dtype, **kw)
        total = (tb["input_ids"] * tb["attention_mask"]).sum()
        assert set(tb.keys()) == set(keys) and all(v.dtype == dtype and v.is_cuda for v in tb.values())
        assert int(total) == int((_shaped(exp, "input_ids", n, width) * _shaped(exp, "attention_mask", n, width)).sum())
        _tensors_equal(tb, exp, n, width, keys)
        tb.sync()
    tb = tk.encode_tensor(list(case["inputs"]), return_token_type_ids=False)
    assert set(tb.keys()) == {"input_ids", "attention_mask"} and len(tb) == 2 and "word_ids" not in tb
    # an empty batch
    assert tuple(tk.encode_tensor([])["input_ids"].shape) == (0, width)
    # a (text, offsets) tensor pair: a tensor that is exactly the text (copied behind the scenes), and a slice of a larger buffer
    buf, off = ta.pack_documents(list(case["inputs"]))
    nb = int(off[-1])
    d_off = torch.from_numpy(np.array(off)).cuda()
    exact = torch.from_numpy(np.array(buf[:nb])).cuda()
    roomy = torch.full((nb + 200,), 0x41, dtype=torch.uint8, device="cuda")
    roomy[:nb] = exact
    for text in (exact, roomy[:nb]):
        tb = tk.encode_tensor((text, d_off), **kw)
        s = tb["attention_mask"].sum(dim=1)
        _tensors_equal(tb, exp, n, width, keys)
        assert s.cpu().tolist() == _shaped(exp, "attention_mask", n, width).sum(axis=1).tolist()
    # pairs
    case = dn.BY_NAME["pairs_bert_longest_left"]
    tk = _tokenizer(case)
    tb = tk.encode_tensor(list(case["inputs"]), **kw)
    types = tb["token_type_ids"].max()
    _tensors_equal(tb, _expect(vectors[case["name"]]), len(case["inputs"]), case["width"], keys)
    assert int(types) == 1


@pytest.mark.needs_hw
def test_encode_tensor_reads_another_tokenizers_decode_tensor(vectors):
    """decode -> encode at the tensor level: A's padded ids -> A.decode_tensor -> B.encode_tensor over the text where it lies; B's rows
    are what B.encode_batch gives for A's decoded strings."""
    import torch
    import tokenizers_amd as ta
    A = ta.Tokenizer.from_str(load_tokenizer_json("bytelevel_prefix_trim_3000"), device=0)
    case = dn.BY_NAME["prefix_only_llama3"]
    B = _tokenizer(case)
    docs = [d for d in dn.docs(40)]
    enc = A.encode_batch_fast(docs, add_special_tokens=False)
    rows = [enc[i].ids for i in range(len(docs))]
    L = max(len(r) for r in rows) + 2
    ids = torch.full((len(docs), L), -100, dtype=torch.int64, device="cuda")
    for r, q in enumerate(rows):
        ids[r, :len(q)] = torch.tensor(q, dtype=torch.int64, device="cuda")
    text = A.decode_tensor(ids)
    tb = B.encode_tensor(text, return_special_tokens_mask=True)
    lens = tb["attention_mask"].sum(dim=1)
    strings = text.to_strings()
    be = B.encode_batch(strings, add_special_tokens=True)
    assert tb["input_ids"].cpu().tolist() == [be[i].ids for i in range(len(be))]
    assert tb["attention_mask"].cpu().tolist() == [be[i].attention_mask for i in range(len(be))]
    assert tb["special_tokens_mask"].cpu().tolist() == [be[i].special_tokens_mask for i in range(len(be))]
    assert lens.cpu().tolist() == [sum(be[i].attention_mask) for i in range(len(be))]


@pytest.mark.needs_hw
def test_encode_tensor_checks_out(vectors):
    import torch
    case = dn.BY_NAME["left_padding"]
    tk = _tokenizer(case)
    n, width = len(case["inputs"]), case["width"]
    docs = list(case["inputs"])
    good = torch.empty((n, width), dtype=torch.int64, device="cuda")
    tb = tk.encode_tensor(docs, out={"input_ids": good, "special_tokens_mask": torch.empty((n, width), dtype=torch.int64, device="cuda")})
    assert tb["input_ids"] is good and "special_tokens_mask" in tb
    _tensors_equal(tb, _expect(vectors[case["name"]]), n, width, ("input_ids", "special_tokens_mask", "attention_mask"))
    for bad, msg in ((torch.empty((n, width + 1), dtype=torch.int64, device="cuda"), "shape"),
                     (torch.empty((n, width), dtype=torch.int32, device="cuda"), "must be torch.int64"),
                     (torch.empty((n, width), dtype=torch.int64), "must live on"),
                     (torch.empty((width, n), dtype=torch.int64, device="cuda").t(), "contiguous")):
        with pytest.raises(ValueError, match=msg):
            tk.encode_tensor(docs, out={"input_ids": bad})
    with pytest.raises(ValueError, match="unknown keys"):
        tk.encode_tensor(docs, out={"ids": good})
    with pytest.raises(ValueError, match="dtype"):
        tk.encode_tensor(docs, dtype=torch.int16)


@pytest.mark.needs_hw
def test_encode_tensor_captured_into_a_graph_and_replayed_over_new_text(vectors):
    """One encode_tensor behind a warm-up call, captured with static text, offsets and output tensors on one stream (one linear chain),
    replayed after the text bytes were overwritten in place with other documents of the same lengths."""
    import torch
    import tokenizers_amd as ta
    case = dn.BY_NAME["prefix_only_llama3"]
    tk = _tokenizer(case)
    docs_a = ["hello world again", "the quick brown fox", "", "abc def"]
    docs_b = ["world hello again", "fox brown quick the", "", "def abc"]
    (buf_a, off), (buf_b, off_b) = ta.pack_documents(docs_a), ta.pack_documents(docs_b)
    assert off.tolist() == off_b.tolist()
    nb, n, width = int(off[-1]), len(docs_a), case["width"]
    store = torch.zeros(nb + 64, dtype=torch.uint8, device="cuda")
    text = store[:nb]
    text.copy_(torch.from_numpy(np.array(buf_a[:nb])))
    d_off = torch.from_numpy(np.array(off)).cuda()
    out = {k: torch.zeros((n, width), dtype=torch.int64, device="cuda") for k in ("input_ids", "attention_mask")}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        tk.encode_tensor((text, d_off), return_token_type_ids=False, out=out).sync()          # warm-up: every buffer has its size
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            keep = tk.encode_tensor((text, d_off), return_token_type_ids=False, out=out)
    torch.cuda.current_stream().wait_stream(side)
    for docs, buf in ((docs_b, buf_b), (docs_a, buf_a)):
        text.copy_(torch.from_numpy(np.array(buf[:nb])).cuda())
        g.replay()
        torch.cuda.synchronize()
        be = tk.encode_batch(docs, add_special_tokens=True)
        assert out["input_ids"].cpu().tolist() == [be[i].ids for i in range(n)], docs
        assert out["attention_mask"].cpu().tolist() == [be[i].attention_mask for i in range(n)]
    del keep
