"""Batches whose TOTAL length is exactly 16,383, 16,384 and 16,385 bytes, as one document and as two: the text's last mask word, the
position n_bytes (where a pre-tokenizer with an end mask puts its last end bit) and the edge of a 256-lane workgroup fall together.
Shared by the CPU tests of the four one-lane-per-word rules (test_pretok_gpt2_words.py, test_digits.py, test_clip.py, test_bloom.py)."""
TOTALS = (16383, 16384, 16385)
UNIT = "it's 12 é。 ٣x, we'll  a.b "      # contractions, digits (ASCII and not), chars of two and three bytes, spaces, punctuation


def _fit(n):
    """n bytes of UNIT repeated, cut at a char edge and filled up with letters"""
    b = (UNIT * (n // len(UNIT.encode("utf-8")) + 2)).encode("utf-8")[:n].decode("utf-8", "ignore")
    return b + "x" * (n - len(b.encode("utf-8")))


def batches(total):
    """[one document of `total` bytes], [two documents of `total` bytes together], and both again with a space as the text's last byte:
    then a whitespace run, not a pre-token, ends exactly at n_bytes, and a pre-tokenizer with an end mask puts no end bit there"""
    first = total // 2 + 1
    out = [[_fit(total)], [_fit(first), _fit(total - first)], [_fit(total - 1) + " "], [_fit(first), _fit(total - first - 1) + " "]]
    assert all(sum(len(d.encode("utf-8")) for d in b) == total for b in out)
    return out
