"""The corpus HostModel::from_json is pinned on (tests/test_host_model_outcomes.py, tools/make_golden_host_model.py), as pure functions:
every tokenizer fixture under tests/golden/, seeds 0..11 of every family of tests/fuzz_cases.py, the cases the differential found, and
two_fault_cases() -- fixtures edited so that TWO refusals of the loader apply, which pins the one that wins: the order the loader asks its
questions in is part of what it answers.  Nothing here imports the library."""
import json
import os
import subprocess

from tests import fuzz_cases as fc
from tests.helpers import load_tokenizer_json

FIXTURES = sorted(fc.FAMILIES + list(fc.HEAVY))
LLAMA3_PATTERN = ("(?i:'s|'t|'re|'ve|'m|'ll|'d)|[^\\r\\n\\p{L}\\p{N}]?\\p{L}+|\\p{N}{1,3}| ?[^\\s\\p{L}\\p{N}]+[\\r\\n]*|\\s*[\\r\\n]+|\\s+(?!\\S)|\\s+")


def _fx(name):
    return json.loads(load_tokenizer_json(name))


def _seq(*types):
    return {"type": "Sequence", "normalizers": [{"type": t} for t in types]}


def _added(content, **props):
    a = {"id": 0, "content": content, "single_word": False, "lstrip": False, "rstrip": False, "normalized": False, "special": False}
    a.update(props)
    return a


def two_fault_cases():
    """name -> tokenizer.json text.  The name says which two refusals meet."""
    out = {}

    d = _fx("bytelevel_prefix_trim_3000")
    d["normalizer"] = _seq("NFKC", "Lowercase")
    out["nfkc_lowercase_sequence__in_front_of_bytelevel"] = d

    d = _fx("nfkc_spm_bpe")
    d["normalizer"] = _seq("NFKC", "Lowercase")
    d["pre_tokenizer"]["split"] = False
    out["nfkc_lowercase_sequence__metaspace_without_split"] = d

    d = _fx("unigram_ms")
    d["normalizer"] = _seq("NFD", "Lowercase")
    d["pre_tokenizer"] = {"type": "ByteLevel", "add_prefix_space": False, "trim_offsets": True, "use_regex": True}
    out["nfd_chain_in_front_of_bytelevel__unigram_model"] = d

    d = _fx("unigram_adv")
    d["normalizer"] = _seq("NFD", "Lowercase")
    d["pre_tokenizer"] = {"type": "Whitespace"}
    out["nfd_chain_in_front_of_whitespace__model_the_chain_is_not_built_for"] = d

    d = _fx("clip_bpe")
    d["pre_tokenizer"]["pretokenizers"][0]["pattern"] = {"Regex": LLAMA3_PATTERN}
    d["model"]["dropout"] = 0.1
    out["clip_normalizer_chain__split_of_another_pattern"] = d

    d = _fx("clip_bpe")
    d["normalizer"] = None
    d["model"]["type"] = "WordPiece"
    out["clip_split_without_the_chain__wordpiece_model"] = d

    d = _fx("spm_bpe_split")
    d["normalizer"] = _fx("precompiled_xlmr")["normalizer"]
    out["precompiled_and_space_runs_replace__bare_metaspace_and_bpe"] = d

    d = _fx("unigram_ms")
    d["pre_tokenizer"] = {"type": "Whitespace"}
    seen = [0]

    def keep(piece):
        if len(piece) == 6 and piece.startswith("<0x") and piece.endswith(">"):
            seen[0] += 1
            return seen[0] <= 100
        return True
    d["model"]["vocab"] = [e for e in d["model"]["vocab"] if keep(e[0])]
    out["unigram_behind_whitespace__100_of_the_256_byte_pieces"] = d

    d = _fx("bloom_bpe")
    d["normalizer"] = {"type": "NFC"}
    d["model"]["type"] = "WordLevel"
    out["bloom_split_behind_nfc__wordlevel_model"] = d

    d = _fx("digits_individual")
    d["normalizer"] = {"type": "BertNormalizer", "clean_text": True, "handle_chinese_chars": True, "strip_accents": None, "lowercase": True}
    d["model"]["type"] = "WordPiece"
    out["digits_bytelevel_behind_bert_normalizer__wordpiece_model"] = d

    d = _fx("bytelevel_prefix_trim_3000")
    d["model"]["dropout"] = 0.1
    del d["model"]["vocab"]["!"]
    out["bpe_dropout__missing_byte_symbol"] = d

    d = _fx("bpe_ws_unk")
    d["post_processor"] = {"type": "ByteLevel", "add_prefix_space": True, "trim_offsets": True, "use_regex": True}
    d["model"]["vocab"][" x"] = len(d["model"]["vocab"])
    d["model"]["type"] = "Foo"
    out["trimming_post_processor_over_a_space_edged_entry__model_type_foo"] = d

    d = _fx("llama3_small_6000")
    d["model"]["end_of_word_suffix"] = "</w>"
    assert d["model"]["ignore_merges"] is True
    out["bytelevel_bpe_with_suffix_and_ignore_merges__no_clip_pre_tokenizer"] = d

    d = _fx("spm_bpe_split")
    d["normalizer"] = _fx("precompiled_ms")["normalizer"]
    d["added_tokens"].append(_added("<n>", normalized=True))
    out["normalized_added_token_behind_precompiled__bpe_model"] = d

    d = _fx("bert_wordpiece_4000")
    d["added_tokens"].append(_added("<far>", id=1 << 25))
    d["truncation"] = {"direction": "Right", "max_length": 16, "strategy": "Foo", "stride": 0}
    out["added_token_id_beyond_2_24__unknown_truncation_strategy"] = d

    d = _fx("spm_bpe_split")
    d["pre_tokenizer"]["split"] = False
    del d["model"]["vocab"]["▁"]
    out["merge_out_of_vocabulary__metaspace_without_split_lacking_u2581"] = d

    # the same meetings from the other side: the fault that lost above stands alone, or a third one joins
    d = _fx("nfkc_spm_bpe")
    d["pre_tokenizer"]["split"] = False
    d["model"]["type"] = "WordPiece"
    out["nfkc_metaspace_without_split__wordpiece_model"] = d

    # (Sequence[NFKC, Lowercase] above reads as a chain with a stranger in it; next to a type that is no chain member it reads as NFKC)
    d = _fx("bytelevel_prefix_trim_3000")
    d["normalizer"] = _seq("NFKC", "Strip")
    out["nfkc_strip_sequence__in_front_of_bytelevel"] = d

    d = _fx("nfkc_spm_bpe")
    d["normalizer"] = _seq("NFKC", "Strip")
    d["pre_tokenizer"]["split"] = False
    out["nfkc_strip_sequence__metaspace_without_split"] = d

    d = _fx("chain_nl_wp")
    d["pre_tokenizer"] = {"type": "Metaspace", "replacement": "▁", "prepend_scheme": "always", "split": True}
    d["model"]["type"] = "Unigram"
    out["nfd_chain_in_front_of_metaspace__unigram_over_an_object_vocab"] = d

    d = _fx("precompiled_xlmr")
    d["pre_tokenizer"]["pretokenizers"][1]["prepend_scheme"] = "first"
    d["added_tokens"].append(_added("<n>", normalized=True))
    out["whitespacesplit_metaspace_prepend_first__normalized_added_token"] = d

    d = _fx("spm_bpe_llama2")
    d["pre_tokenizer"] = {"type": "Whitespace"}
    d["added_tokens"].append(_added("<n>", normalized=True))
    out["u2581_normalizers_in_front_of_whitespace__normalized_added_token"] = d

    d = _fx("ds3_chain")
    d["normalizer"] = {"type": "BertNormalizer"}
    d["model"]["byte_fallback"] = True
    out["chained_split_behind_bert_normalizer__bytelevel_byte_fallback"] = d

    d = _fx("bpe_ws_byte_fallback")
    d["model"]["continuing_subword_prefix"] = "##"
    del d["model"]["vocab"]["<0x41>"]
    out["byte_fallback_with_affix__missing_byte_token"] = d

    d = _fx("nfc_gpt2")
    d["pre_tokenizer"]["add_prefix_space"] = True
    d["model"]["type"] = "WordLevel"
    out["nfc_bytelevel_prefix_space__wordlevel_model"] = d
    return {k: json.dumps(v, ensure_ascii=False) for k, v in out.items()}


def groups():
    """group -> [(key, tokenizer.json text)], lazily: a fixture with its twelve seeded edits (the seven HEAVY fixtures alone), the found
    cases, the two-fault list.  The keys are those of tests/golden/host_model_outcomes.json.gz."""
    def fixture(name):
        yield f"fixture/{name}", load_tokenizer_json(name)
        if name not in fc.HEAVY:
            for seed in fc.SEEDS:
                yield f"fuzz/{name}/{seed}", fc.make_case(name, seed)["json"]

    def found():
        for finding, cases in sorted(fc.found_cases().items()):
            for k, case in enumerate(cases):
                yield f"found/{finding}/{k}", case["json"]

    def two_fault():
        for name, js in sorted(two_fault_cases().items()):
            yield f"two_fault/{name}", js

    out = {name: (lambda name=name: fixture(name)) for name in FIXTURES}
    out["found"] = found
    out["two_fault"] = two_fault
    return out


GROUPS = groups()


def parse_line(line, layout=False):
    """one line of tests/harness/host_model_digest.cpp -> (key, what the golden file records of it): status and message, or status and
    the config and content digests (the layout digest belongs to one libstdc++: not recorded)"""
    cols = line.rstrip("\n").split("\t")
    if cols[1] == "OK":
        return cols[0], {"status": "OK", "config": cols[2], "content": cols[3], **({"layout": cols[4]} if layout else {})}
    return cols[0], {"status": cols[1], "message": cols[2]}


# ---------------------------------------------------------------------------------------------------------------------------------
# Building and running the harness (shared by the test and by tools/make_golden_host_model.py)
# ---------------------------------------------------------------------------------------------------------------------------------
HERE =os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "tokenizers_amd", "csrc")
SRCS = [os.path.join(HERE, "harness", "host_model_digest.cpp"), os.path.join(CSRC, "host_model.cpp")]


def build_harness(exe, flags=("-O2",), host_model_cpp=None):
    """g++ [flags] -std=c++17 -I tokenizers_amd/csrc host_model_digest.cpp host_model.cpp -o exe (host_model_cpp: another copy of that file)"""
    srcs = [SRCS[0], host_model_cpp or SRCS[1]]
    tmp = f"{exe}.{os.getpid()}.tmp"
    subprocess.run(["g++", *flags, "-std=c++17", "-I" + CSRC] + srcs + ["-o", tmp], check=True)
    os.replace(tmp, exe)
    return exe


def run_harness(exe, items, workdir, jobs=None, layout=False):
    """the harness's answers to [(key, tokenizer.json text)] as {key: record}; the files are written under workdir, the list is dealt
    round-robin to `jobs` processes"""
    items = list(items)
    jobs = max(1, min(jobs or min(8, os.cpu_count() or 1), len(items)))
    lists = []
    for j in range(jobs):
        lists.append(os.path.join(workdir, f"list{j}.txt"))
        with open(lists[-1], "w", encoding="utf-8") as fh:
            for k in range(j, len(items), jobs):
                path = os.path.join(workdir, f"{k}.json")
                with open(path, "w", encoding="utf-8") as out:
                    out.write(items[k][1])
                fh.write(f"{items[k][0]}\t{path}\n")
    procs = [subprocess.Popen([exe, "--list", p], stdout=subprocess.PIPE, text=True, encoding="utf-8") for p in lists]
    got = {}
    for p in procs:
        text, _ = p.communicate()
        assert p.returncode == 0, (p.returncode, text[-2000:])
        got.update(parse_line(line, layout) for line in text.splitlines())
    assert list(got) and len(got) == len(items), (len(got), len(items))
    return got
