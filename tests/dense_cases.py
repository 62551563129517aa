"""The cases of the dense entry (tkamd_encode_batch_device_dense, Tokenizer.encode_tensor) as a pure module: nothing here imports the
library or the wheel.  tools/make_golden_dense.py records the wheel's answer for every case -- per Encoding the stacked ids,
attention_mask, type_ids, special_tokens_mask, offsets and word_ids (None -> -1) -- in tests/golden/dense_vectors.json.gz;
tests/test_dense_gpu.py holds the device to them.

A case is a tokenizer fixture, optionally another post-processor, a `truncation` and a `padding` section (Fixed: the dense entry's
condition) and a batch of single sequences or pairs whose FIRST input is the one the case is about; the tests also run that input alone.
Under Fixed padding every encoding stands on its own, so the wheel's answer for inputs[:n] is the first n rows of its answer for the
batch: the shape matrix (every width x every number of rows) is recorded once per width, for the longest batch."""
import json

from tests.helpers import load_tokenizer_json

WIDTHS = (1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 63, 64, 65)
ROWS = (0, 1, 2, 3, 255, 256, 257)
FIELDS = ("input_ids", "attention_mask", "token_type_ids", "special_tokens_mask", "offset_mapping", "word_ids")

BERT = "bert_wordpiece_4000_specials"
BYTELEVEL = "bytelevel_prefix_trim_3000"
L3S = "llama3_small_6000_specials"
SPM = "spm_bpe_llama2"
UNIGRAM = "unigram_ms"

_SEED_DOCS = ["The quick brown fox jumps over the lazy dog.", "", "café naïve 中文 Жук \U0001F600 ok", "some counterrevolutionaries here",
              "supercalifragilisticexpialidociousnesses", "b" + "ab" * 35 + " end", "It's 2024, isn't it? Yes!!", "  leading and trailing  ",
              "tabs\tand\nnewlines\r\n", "hello hello hello world world", "A", "MixedCase camelCaseWord HTTPServer's", "x",
              "one two three four five six seven eight nine ten eleven twelve thirteen fourteen fifteen sixteen seventeen eighteen nineteen twenty "
              "twenty-one twenty-two twenty-three twenty-four twenty-five twenty-six twenty-seven twenty-eight twenty-nine thirty thirty-one "
              "thirty-two thirty-three thirty-four thirty-five thirty-six thirty-seven thirty-eight thirty-nine forty"]
LONG = _SEED_DOCS[-1]


def docs(n: int) -> list:
    """n documents of every length class: the seed documents, then each again behind a growing head of words"""
    out = []
    k = 0
    while len(out) < n:
        s = _SEED_DOCS[k % len(_SEED_DOCS)]
        r = k // len(_SEED_DOCS)
        out.append(s if r == 0 else " ".join(["w%d" % (r + j) for j in range(r % 9)] + [s]))
        k += 1
    return out


def _trunc(max_length, strategy="LongestFirst", direction="Right", stride=0):
    return {"direction": direction, "max_length": max_length, "strategy": strategy, "stride": stride}


def _pad(length, direction="Right", multiple=None, pad_id=0, pad_type_id=0, pad_token="[PAD]"):
    return {"strategy": {"Fixed": length}, "direction": direction, "pad_to_multiple_of": multiple, "pad_id": pad_id, "pad_type_id": pad_type_id,
            "pad_token": pad_token}


def _case(name, tokenizer, inputs, trunc, pad, width, add_special=True, post=None):
    return dict(name=name, tokenizer=tokenizer, inputs=inputs, truncation=trunc, padding=pad, width=width, add_special_tokens=add_special, post=post,
                pairs=bool(inputs) and isinstance(inputs[0], tuple))


ROBERTA = {"type": "RobertaProcessing", "sep": ["</s>", 2], "cls": ["<s>", 1], "trim_offsets": True, "add_prefix_space": True}
TYPED = {"type": "TemplateProcessing",
         "single": [{"SpecialToken": {"id": "[CLS]", "type_id": 0}}, {"Sequence": {"id": "A", "type_id": 1}}, {"SpecialToken": {"id": "[SEP]", "type_id": 1}}],
         "pair": [{"SpecialToken": {"id": "[CLS]", "type_id": 0}}, {"Sequence": {"id": "A", "type_id": 0}}, {"SpecialToken": {"id": "[SEP]", "type_id": 0}},
                  {"Sequence": {"id": "B", "type_id": 1}}, {"SpecialToken": {"id": "[SEP]", "type_id": 1}}],
         "special_tokens": {"[CLS]": {"id": "[CLS]", "ids": [2], "tokens": ["[CLS]"]}, "[SEP]": {"id": "[SEP]", "ids": [3], "tokens": ["[SEP]"]}}}

SHORT = ["A", "", "hello world", LONG, "café 中文", "It's 2024"]
# pairs for every strategy: both long (LongestFirst), a long first with a short second (OnlyFirst), the other way round (OnlySecond)
PAIRS_BOTH = [(LONG, LONG[40:]), ("", ""), ("A", "hello world"), ("", "x"), ("hello hello hello world", ""), ("café 中文", "It's 2024, isn't it? Yes!!")]
PAIRS_FIRST = [(LONG, "short one"), ("", ""), ("A", "b"), (LONG[30:], ""), ("x", "hello world")]
PAIRS_SECOND = [("short one", LONG), ("", ""), ("A", "b"), ("", LONG[30:]), ("hello world", "x")]


def _cases():
    out = []
    # the shape matrix: every width, 257 rows (tests take the first n of them for every n of ROWS); below two columns there is no room
    # for [CLS] and [SEP]
    for w in WIDTHS:
        out.append(_case("shape_w%d" % w, BERT, docs(max(ROWS)), _trunc(w), _pad(w), w, add_special=w >= 2))
    # n_rows x width beyond one grid's share of elements on the device (2048 workgroups x 256 lanes x 2 int64 elements)
    out.append(_case("shape_grid", BERT, docs(8200), _trunc(128), _pad(128), 128))
    out += [
        _case("left_padding", BERT, SHORT, _trunc(16), _pad(16, direction="Left", pad_id=7, pad_type_id=1), 16),
        _case("pad_multiple", BERT, SHORT, _trunc(12), _pad(12, multiple=8), 16),
        _case("truncate_left", BERT, [LONG] + SHORT, _trunc(9, direction="Left"), _pad(9), 9),
        _case("exact_width", BERT, [LONG, "A"], _trunc(17), _pad(17), 17),
        _case("empty_with_specials", BERT, ["", "A", ""], _trunc(5), _pad(5, pad_id=9), 5),
        _case("empty_plain", BERT, ["", "A", ""], _trunc(5), _pad(5, pad_id=9), 5, add_special=False),
        _case("no_specials", BERT, [LONG] + SHORT, _trunc(15), _pad(15), 15, add_special=False),
        _case("no_specials_left", L3S, [LONG] + SHORT, _trunc(15, direction="Left"), _pad(17, direction="Left", pad_id=5), 17, add_special=False),
        _case("typed_single", BERT, [LONG] + SHORT, _trunc(16), _pad(16, pad_type_id=2), 16, post=TYPED),
        _case("typed_single_left", BERT, SHORT, _trunc(16), _pad(16, direction="Left", pad_type_id=2), 16, post=TYPED),
        _case("pairs_bert_longest", BERT, PAIRS_BOTH, _trunc(16), _pad(16), 16),
        _case("pairs_bert_longest_left", BERT, PAIRS_BOTH, _trunc(15, direction="Left"), _pad(17, direction="Left", pad_type_id=1), 17),
        _case("pairs_bert_only_first", BERT, PAIRS_FIRST, _trunc(16, strategy="OnlyFirst"), _pad(16), 16),
        _case("pairs_bert_only_second", BERT, PAIRS_SECOND, _trunc(16, strategy="OnlySecond"), _pad(16), 16),
        _case("pairs_bert_plain", BERT, PAIRS_BOTH, _trunc(16), _pad(16), 16, add_special=False),
        _case("pairs_roberta_longest", BYTELEVEL, PAIRS_BOTH, _trunc(16), _pad(16, pad_id=3), 16, post=ROBERTA),
        _case("pairs_roberta_only_first", BYTELEVEL, PAIRS_FIRST, _trunc(16, strategy="OnlyFirst"), _pad(16, pad_id=3), 16, post=ROBERTA),
        _case("pairs_roberta_only_second", BYTELEVEL, PAIRS_SECOND, _trunc(16, strategy="OnlySecond"), _pad(16, pad_id=3), 16, post=ROBERTA),
        _case("roberta_single", BYTELEVEL, [LONG] + SHORT, _trunc(16), _pad(16, pad_id=3), 16, post=ROBERTA),
        _case("bytelevel_plain", BYTELEVEL, [LONG] + SHORT, _trunc(16), _pad(16, pad_id=3), 16, add_special=False),
        _case("prefix_only_spm", SPM, [LONG] + SHORT, _trunc(16), _pad(16), 16),
        _case("prefix_only_spm_pairs", SPM, PAIRS_BOTH, _trunc(16), _pad(16), 16),
        _case("prefix_only_llama3", L3S, [LONG] + SHORT, _trunc(16), _pad(16, pad_id=5), 16),
        _case("prefix_only_min", SPM, ["", "A", LONG], _trunc(1), _pad(1), 1),
        _case("unigram", UNIGRAM, [LONG] + SHORT, _trunc(16), _pad(16), 16),
        _case("unigram_left", UNIGRAM, SHORT, _trunc(7, direction="Left"), _pad(8, direction="Left", multiple=4), 8),
    ]
    return out


CASES = _cases()
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
SHAPE_CASES = ["shape_w%d" % w for w in WIDTHS]
# recorded by digest only (the vectors would be 8200 x 128 x 7 numbers)
DIGEST_ONLY = ("shape_grid",)


def tokenizer_json(case) -> str:
    """the fixture's JSON with the case's post-processor, truncation and padding sections"""
    d = json.loads(load_tokenizer_json(case["tokenizer"]))
    if case["post"] is not None:
        d["post_processor"] = case["post"]
    d["truncation"] = case["truncation"]
    d["padding"] = case["padding"]
    return json.dumps(d, ensure_ascii=False)
