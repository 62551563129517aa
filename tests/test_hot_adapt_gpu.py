"""-m gpu: the hot-word table that learns the handle's text (csrc/capi/tables.cpp hot_census_read, kernels/lookup.hip k_hot_census) on the
MI355X, with the test hooks TKAMD_HOT_CENSUS_MIN_BYTES / TKAMD_HOT_CENSUS_PERIOD so that batches of a few hundred KB are eligible.

  * the results of a batch do not depend on the table: checksums of ids and token CSR (and of char offsets and word ids) are equal with
    the adaptation off, on before any census, on the batch that takes the census and after the rebuild -- GPT-2 ids-only, GPT-2 with char
    offsets and word ids, BERT, Llama-3;
  * text whose words stay what they were rebuilds the table once: the next census finds nothing to gain;
  * the table learns the distribution, not the batch: rebuilt from a census of 1 MiB of one text it settles at least ten points more of
    the pre-tokens of 1 MiB of ANOTHER text of the same distribution than the load-time table does, by the same counter;
  * two threads on two streams encode through one handle while the table is rebuilt under them: every result equals the oracle's;
  * TKAMD_HOT_ADAPT=0 never launches the census."""
import threading

import numpy as np
import pytest

from oracle import oracle as orc
from oracle import synth
from tests.helpers import load_tokenizer_json

pytestmark = [pytest.mark.gpu, pytest.mark.needs_hw]            # (torch device tensors hold the resident batches)

MIN_BYTES = 65536


def _hooks(monkeypatch, period, min_bytes=MIN_BYTES, adapt=None):
    monkeypatch.setenv("TKAMD_TEST_HOOKS", "1")
    monkeypatch.setenv("TKAMD_HOT_CENSUS_MIN_BYTES", str(min_bytes))
    monkeypatch.setenv("TKAMD_HOT_CENSUS_PERIOD", str(period))
    if adapt is None:
        monkeypatch.delenv("TKAMD_HOT_ADAPT", raising=False)
    else:
        monkeypatch.setenv("TKAMD_HOT_ADAPT", adapt)


def _json(name):
    return synth.load_or_train_gpt2() if name == "gpt2" else load_tokenizer_json(name)


class Resident:
    """documents packed and resident in HBM"""

    def __init__(self, docs):
        import torch
        import tokenizers_amd as ta
        buf, off = ta.pack_documents(docs)
        self.n_docs, self.n_bytes = len(docs), int(off[-1])
        self.d_text, self.d_off = torch.from_numpy(np.array(buf)).cuda(), torch.from_numpy(np.array(off)).cuda()

    def run(self, tok, stream=None, **kw):
        import torch
        st = torch.cuda.current_stream().cuda_stream if stream is None else stream
        return tok.encode_batch_device(self.d_text.data_ptr(), self.d_off.data_ptr(), self.n_docs, self.n_bytes, stream=st, **kw).sync()


def _lines_of(n_bytes, text_seed):
    """lines of the bench's own corpus, a little more than n_bytes of them"""
    lines, total, out = synth.gen_lines(n_bytes // 100, text_seed=text_seed), 0, []
    for l in lines:
        out.append(l)
        total += len(l.encode("utf-8"))
        if total >= n_bytes:
            return out
    raise AssertionError("gen_lines gave less text than asked for")


def _checksum(b, meta):
    """sums and position-weighted sums of everything the call returned (bench.py result_checksum, with the offsets and word ids)"""
    import torch
    arrays = [b.ids_tensor().to(torch.int64), b.tok_offsets_tensor()]
    if meta:
        arrays += [b.offsets_tensor().to(torch.int64).flatten(), b.word_ids_tensor().to(torch.int64)]
    out = [int(b.n_tokens)]
    for a in arrays:
        w = (torch.arange(a.numel(), dtype=torch.int64, device=a.device) % 1000003) + 1
        out += [int(a.numel()), int(a.sum()), int((a * w).sum())]
    return tuple(out)


@pytest.mark.parametrize("name,kw", [("gpt2", {}), ("gpt2", dict(offsets="char", word_ids=True)), ("bert_wordpiece_4000", {}), ("llama3_small_6000", {})],
                         ids=["gpt2_ids", "gpt2_char_offsets_words", "bert", "llama3"])
def test_results_do_not_depend_on_the_table(name, kw, monkeypatch):
    import tokenizers_amd as ta
    js = _json(name)
    batch = Resident(_lines_of(300_000, text_seed=100) + ["", "café naïve 中文 Жук ok", "x" * 300])
    meta = bool(kw)
    _hooks(monkeypatch, period=3, adapt="0")
    off = ta.Tokenizer.from_str(js, device=0)
    want = _checksum(batch.run(off, **kw), meta)
    assert off.info["hot_census_sample"] == 0 and not off.info["hot_adapt"]
    _hooks(monkeypatch, period=3, min_bytes=1 << 30)            # on, and this batch is below the threshold: no census yet
    early = ta.Tokenizer.from_str(js, device=0)
    assert _checksum(batch.run(early, **kw), meta) == want
    assert early.info["hot_adapt"] and early.info["hot_census_sample"] == 0
    _hooks(monkeypatch, period=3)
    tok = ta.Tokenizer.from_str(js, device=0)
    assert _checksum(batch.run(tok, **kw), meta) == want           # the batch that takes the census
    info = tok.info
    assert info["hot_census_sample"] > 0 and info["hot_generation"] == 1, info
    assert info["hot_rate_selected"] >= info["hot_rate_in_use"] + 0.02, info
    for _ in range(3):                                              # after the rebuild (the third of them takes the next census)
        assert _checksum(batch.run(tok, **kw), meta) == want
    assert tok.info["hot_generation"] == 1


def test_stationary_text_rebuilds_the_table_once(monkeypatch):
    import tokenizers_amd as ta
    _hooks(monkeypatch, period=2)
    tok = ta.Tokenizer.from_str(_json("gpt2"), device=0)
    seen = []
    for k in range(5):                                              # censuses on batches 0, 2 and 4, each over other lines of the same distribution
        Resident(_lines_of(400_000, text_seed=100 + k)).run(tok)
        seen.append(tok.info)
    assert [i["hot_generation"] for i in seen] == [1, 1, 1, 1, 1], seen
    assert seen[0]["hot_census_sample"] == seen[1]["hot_census_sample"] != seen[2]["hot_census_sample"], "batch 2 took no census of its own"
    for i in (seen[2], seen[4]):                                    # what the rebuilt table settles of NEW text is what the census promised, and nothing is left to gain
        assert i["hot_rate_in_use"] >= seen[0]["hot_rate_selected"] - 0.03, (i, seen[0])
        assert i["hot_rate_selected"] < i["hot_rate_in_use"] + 0.02, i


def test_the_table_learns_the_distribution_not_the_batch(monkeypatch):
    """(the condition of the change: a CPU simulation of the rule gives 14.5 points on these texts; a table that memorised its sample fails)"""
    import tokenizers_amd as ta
    js = _json("gpt2")
    train, held_out = Resident(_lines_of(1 << 20, text_seed=100)), Resident(_lines_of(1 << 20, text_seed=1100))
    _hooks(monkeypatch, period=1, min_bytes=1 << 20)
    base = ta.Tokenizer.from_str(js, device=0)
    held_out.run(base)
    load_time_rate = base.info["hot_rate_in_use"]                   # the load-time table, on the held-out text
    tok = ta.Tokenizer.from_str(js, device=0)
    train.run(tok)
    assert tok.info["hot_generation"] == 1
    held_out.run(tok)
    learned_rate = tok.info["hot_rate_in_use"]                      # the table rebuilt from the OTHER text, same counter, same text
    print("sampled hit rate on 1 MiB of held-out text: load-time table %.4f, learned table %.4f (sample %d pre-tokens)"
          % (load_time_rate, learned_rate, tok.info["hot_census_sample"]))
    assert base.info["hot_census_sample"] == tok.info["hot_census_sample"] > 100_000
    assert learned_rate >= load_time_rate + 0.10


def test_two_streams_encode_through_one_handle_across_a_rebuild(monkeypatch):
    import torch
    import tokenizers_amd as ta
    js = _json("gpt2")
    _hooks(monkeypatch, period=2)
    tok, o = ta.Tokenizer.from_str(js, device=0), orc.Oracle(js)
    docs = [_lines_of(250_000, text_seed=100) + ["", "it's"], _lines_of(250_000, text_seed=101) + ["x" * 500]]
    exp = [o.encode_batch(d) for d in docs]
    batches = [Resident(d) for d in docs]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    bad, errors = [], []

    def worker(k):
        try:
            torch.cuda.set_device(0)
            for rep in range(6):
                b = batches[k].run(tok, stream=streams[k].cuda_stream)
                ids = b.ids_tensor().cpu().numpy().view(np.uint32)
                if not (np.array_equal(b.tok_offsets_tensor().cpu().numpy(), exp[k].tok_offsets) and np.array_equal(ids, exp[k].ids)):
                    bad.append((k, rep))
        except Exception as e:      # noqa: BLE001 (reported by the assertion below)
            errors.append(repr(e))

    threads = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert not bad, bad
    assert tok.info["hot_generation"] >= 1, tok.info                # (a rebuild did happen under them)


def test_switched_off_in_the_environment_no_census_is_launched(monkeypatch):
    import tokenizers_amd as ta
    js = _json("gpt2")
    batch = Resident(_lines_of(200_000, text_seed=100))
    for adapt, expect in (("0", False), (None, True)):
        _hooks(monkeypatch, period=1, adapt=adapt)
        tok = ta.Tokenizer.from_str(js, device=0)
        tok.profile(True)
        batch.run(tok)
        batch.run(tok)
        stages = tok.profile_read()
        assert ("hot_census" in stages) == expect, stages
        assert "lookup" in stages
