"""What k_hot_census (csrc/kernels/lookup.hip) must count for a batch, recounted in Python from the reference's own normalizer and
pre-tokenizer: the sample's tiles, the pre-tokens that start in them, and which of those are eligible words of the hot table.
Shared by tests/test_hot_census_simt.py and tests/test_hot_adapt_gpu.py; test infrastructure only."""
import json

TILE = 16384          # LU_TILE: bytes of X text per tile
TILES = 64            # HC_TILES: tiles a census samples
HOT_MAX_KEY = 12


def sample_tiles(n_bytes: int) -> list[int]:
    """the tiles a census of n_bytes of X text samples (hot_census_tile)"""
    n_tiles = (((n_bytes + 63) >> 6) + 255) // 256
    n_sample = min(TILES, n_tiles)
    return [i * n_tiles // n_sample for i in range(n_sample)]


def _byte_level_table():
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAD)) + list(range(0xAE, 0x100))
    cs, n = bs[:], 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return {chr(c): b for b, c in zip(bs, cs)}


def token_bytes(tok_json: str) -> dict[int, bytes]:
    """id -> the bytes of the X text a whole-word hit of that token stands for"""
    d = json.loads(tok_json)
    vocab = d["model"]["vocab"]
    pre = d.get("pre_tokenizer") or {}
    kinds = [pre.get("type")] + [p.get("type") for p in pre.get("pretokenizers", [])]
    if "ByteLevel" in kinds:
        u2b = _byte_level_table()
        return {i: bytes(u2b[c] for c in t) for t, i in vocab.items() if all(c in u2b for c in t)}
    return {i: t.encode("utf-8") for t, i in vocab.items()}


def pretokens(ref_tok, docs: list[str]):
    """(start, end) in bytes of the X text -- the documents' normalized texts, concatenated -- of every pre-token, and that text"""
    out, base, x = [], 0, []
    for doc in docs:
        nd = ref_tok.normalizer.normalize_str(doc) if ref_tok.normalizer is not None else doc
        c2b = [0]
        for ch in nd:
            c2b.append(c2b[-1] + len(ch.encode("utf-8")))
        for _, (s, e) in ref_tok.pre_tokenizer.pre_tokenize_str(nd):
            out.append((base + c2b[s], base + c2b[e]))
        x.append(nd.encode("utf-8"))
        base += c2b[-1]
    return out, b"".join(x)


def recount(ref_tok, tok_json: str, docs: list[str], eligible_ids) -> tuple[dict[int, int], int]:
    """({id: sampled pre-tokens that are that eligible word}, sampled pre-tokens) of one batch"""
    pts, x = pretokens(ref_tok, docs)
    tiles = set(sample_tiles(len(x)))
    eligible = set(eligible_ids)
    by_bytes = {b: i for i, b in token_bytes(tok_json).items() if i in eligible}
    counts, total = {}, 0
    for s, e in pts:
        if e == s or s // TILE not in tiles:
            continue
        total += 1
        i = by_bytes.get(x[s:e]) if e - s <= HOT_MAX_KEY else None
        if i is not None:
            counts[i] = counts.get(i, 0) + 1
    return counts, total
