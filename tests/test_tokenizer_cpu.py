"""The CLIP BPE tokenizer and the prompt assembly at the C ABI, the part that needs no GPU.  The oracle is transformers' CLIPTokenizer
built from the same synthetic vocab.json / merges.txt (tests/tokenizer_ref.py); every comparison is an equality."""
import ctypes as C
import random
import re

import pytest
import torch

from edgestyle_amd import lib as L
from edgestyle_amd.lib import EdgeStyleHipError
from edgestyle_amd.prompts import DEFAULT_CLOTHING_ITEMS, DEFAULT_COLORS
from edgestyle_amd.tokenizer import NativeCLIPTokenizer
from tests import tokenizer_ref as R

NEW_SYMBOLS = ("es_tokenizer_create", "es_tokenizer_create_from_memory", "es_tokenizer_destroy", "es_tokenizer_vocab_size",
               "es_tokenizer_max_length", "es_tokenizer_bos_id", "es_tokenizer_eos_id", "es_tokenizer_pad_id", "es_tokenize", "es_tokenize_padded",
               "es_prompt_table_create", "es_prompt_table_destroy", "es_prompt_assemble", "es_prompt_assemble_host", "es_text_encode_dev")
KW = dict(padding="max_length", truncation=True, return_tensors="pt")


class Case:
    def __init__(self, directory, holes, max_length=77):
        self.vp, self.mp = R.write_files(directory, holes=holes, escape=not holes)      # the holed vocabulary is saved as raw UTF-8
        self.L = max_length
        self.oracle = R.oracle(self.vp, self.mp, max_length)
        self.native = NativeCLIPTokenizer(self.vp, self.mp, max_length)

    def same(self, texts):
        """the texts whose native row differs from the oracle's (none was refused: a refusal raises)"""
        want = R.oracle_ids(self.oracle, texts, self.L)
        got = self.native(texts, max_length=self.L, **KW).input_ids
        assert got.dtype == torch.int64 and got.shape == want.shape
        return [t for t, a, b in zip(texts, want, got) if not torch.equal(a, b)]


@pytest.fixture(scope="module")
def full(tmp_path_factory):
    return Case(tmp_path_factory.mktemp("tok_full"), holes=False)


@pytest.fixture(scope="module")
def holed(tmp_path_factory):
    return Case(tmp_path_factory.mktemp("tok_holes"), holes=True)


def test_abi_version_is_unchanged_and_the_new_symbols_resolve():
    lib = L.load()
    assert lib.es_abi_version() == 7
    for name in NEW_SYMBOLS:
        assert name in L.SYMBOLS and getattr(lib, name)


def test_attributes_are_the_oracles(full, holed):
    for c in (full, holed):
        n, o = c.native, c.oracle
        assert (n.bos_token_id, n.eos_token_id, n.pad_token_id) == (o.bos_token_id, o.eos_token_id, o.pad_token_id)
        assert n.vocab_size == len(o) and n.model_max_length == o.model_max_length == 77
        assert n.lib.es_tokenizer_max_length(n._h) == 77


def _token_count(c, text):
    return len(c.oracle(text, add_special_tokens=False).input_ids)


def _texts_of_exactly(c, counts):
    """one text per requested token count, grown word by word (single digits are one token each: any count can be hit)"""
    rng, out = random.Random(5), []
    words = DEFAULT_COLORS + DEFAULT_CLOTHING_ITEMS + ["it's", "3", "...", "wearing"]
    for want in counts:
        text = ""
        while _token_count(c, text) < want - 1:
            nxt = text + (" " if text else "") + rng.choice(words)
            if _token_count(c, nxt) > want:
                break
            text = nxt
        while _token_count(c, text) < want:
            text += " 7"
        assert _token_count(c, text) == want
        out.append(text)
    return out


def test_fixed_cases_equal_the_oracle(full, holed):
    words = DEFAULT_COLORS + DEFAULT_CLOTHING_ITEMS
    rng = random.Random(2)
    prompts = ["edgestyle, " + ", ".join(rng.sample(DEFAULT_COLORS, 2) + rng.sample(DEFAULT_CLOTHING_ITEMS, 2)) + " best quality" for _ in range(40)]
    fixed = ["", " ", "\t\n\v\f\r", " \t a \n\n b\v\fc\r ", "it's they're we've i'm he'll she'd isn't", "IT'S THEY'RE 'S 'T 'RE 'VE 'M 'LL 'D 'l 'r 'v",
             "a's'tb x'' ''s !'s 'sx 'lly 'dd", "0123456789", "3.14 100% 10-20 7up 4x4 a1b2", "!!!", "...???,,,", "(a) [b] {c} <d> a|b <| |>", "~`@#$%^&*_+-=\\/\"",
             "MiXeD CaSe ShIrT", "<|start of text|> <|endoftex|> <startoftext>", "t-shirt!, x", "t-shirt! , x"]
    for c in (full, holed):
        texts = words + prompts + fixed + _texts_of_exactly(c, range(74, 79))
        assert c.same(texts) == []
        # the untruncated ids too, and the first-EOS position of every padded row
        for t in fixed + prompts[:5]:
            assert c.native.tokenize_ids(t) == c.oracle(t, add_special_tokens=False).input_ids, t
        ids, eos = c.native.padded(texts, with_eos=True)
        assert eos.tolist() == (ids == c.native.eos_token_id).int().argmax(dim=1).tolist()
    # in the holed vocabulary the unk path really ran: an unk id in front of the closing EOS
    ids, eos = holed.native.padded(["quiz", "zebra"], with_eos=True)
    assert eos.tolist() == [1, 1] and bool((ids[:, 2:6] != holed.native.eos_token_id).any(dim=1).all())


def test_the_truncated_row_keeps_its_eos(full):
    t74, t75, t76 = _texts_of_exactly(full, [74, 75, 76])
    ids = full.native([t74, t75, t76], max_length=77, **KW).input_ids
    eos = full.native.eos_token_id
    assert ids[0, 75].item() == eos and ids[0, 74].item() != eos            # 74 tokens: EOS at 75, one pad
    assert ids[1, 76].item() == eos and ids[1, 75].item() != eos            # 75 tokens fill the row
    assert ids[2, 76].item() == eos and torch.equal(ids[2, :76], torch.tensor([full.native.bos_token_id] + full.native.tokenize_ids(t76)[:75]))


@pytest.mark.parametrize("which", ["full", "holed"])
def test_random_sweep_over_the_accepted_bytes(which, full, holed):
    c = full if which == "full" else holed
    texts = R.random_texts(2200, seed=11 if which == "full" else 12)
    assert len(texts) >= 2000 and max(map(len, texts)) > 290 and "" in texts
    assert all(set(t.encode()) <= set(R.ACCEPTED) for t in texts)
    seen = set().union(*(set(t.encode()) for t in texts))
    assert seen == set(R.ACCEPTED)                                           # every accepted byte occurs
    assert c.same(texts) == []                                               # none refused (that raises), none different
    # short rows are compared whole above; long ones only up to the cut, so the untruncated ids of some of them as well
    for t in texts[:200]:
        assert c.native.tokenize_ids(t) == c.oracle(t, add_special_tokens=False).input_ids, t


def test_other_max_lengths(tmp_path):
    for Lm in (2, 3, 8, 16):
        c = Case(tmp_path / f"L{Lm}", holes=False, max_length=Lm)
        assert c.same(["", "red", "a polo shirt, a tank top", "1234567890123456"]) == []


@pytest.mark.parametrize("text,reason", [
    (b"caf\xc3\xa9", r"byte 0xC3 at offset 3 is outside the accepted set"),
    (b"a\x00b", r"byte 0x00 at offset 1"),
    (b"ab\x7f", r"byte 0x7F at offset 2"),
    (b"\x1f", r"byte 0x1F at offset 0"),
    (b"x <|endoftext|>", r"special token literal '<\|endoftext\|>' at offset 2"),
    (b"<|startoftext|>x", r"special token literal '<\|startoftext\|>' at offset 0"),
    (b"a <|EndOfText|>", r"special token literal '<\|endoftext\|>' at offset 2"),
])
def test_refused_texts(full, text, reason):
    with pytest.raises(EdgeStyleHipError, match=reason):
        full.native.tokenize_ids(text)
    with pytest.raises(EdgeStyleHipError, match=reason):
        full.native([text], **KW)
    if b"\xc3" in text:
        with pytest.raises(EdgeStyleHipError, match=reason):
            full.native("café", **KW)


def test_unsupported_call_forms_raise(full):
    for kw in (dict(padding=True, truncation=True, return_tensors="pt"), dict(padding="max_length", truncation=True),
               dict(padding="max_length", truncation=True, return_tensors="pt", max_length=20),
               dict(padding="max_length", truncation=True, return_tensors="pt", return_attention_mask=True)):
        with pytest.raises(EdgeStyleHipError):
            full.native("red", **kw)


def _create(vocab: bytes, merges: bytes, max_length=77):
    lib, h = L.load(), C.c_void_p()
    rc = lib.es_tokenizer_create_from_memory(vocab, len(vocab), merges, len(merges), max_length, C.byref(h))
    if rc == 0:
        lib.es_tokenizer_destroy(h)
    return rc, lib.es_last_error().decode()


def test_loader_errors_name_the_line_or_key(full, tmp_path):
    vocab, merges = open(full.vp, "rb").read(), open(full.mp, "rb").read()
    assert _create(vocab, merges)[0] == 0
    rc, msg = _create(vocab, merges, max_length=1)
    assert rc == -1 and "max_length = 1 is below 2" in msg
    lines = merges.decode().splitlines()
    rc, msg = _create(vocab, ("\n".join(lines[:3] + ["e qq"] + lines[3:]) + "\n").encode())
    assert rc == -1 and "merges.txt line 4: 'qq' is not in the vocabulary" in msg
    rc, msg = _create(vocab, ("\n".join(lines + ["q j"]) + "\n").encode())                  # both parts exist, their result does not
    assert rc == -1 and f"merges.txt line {len(lines) + 1}: 'qj' is not in the vocabulary" in msg
    rc, msg = _create(vocab, ("\n".join(lines + ["a b c"]) + "\n").encode())
    assert rc == -1 and f"merges.txt line {len(lines) + 1}: expected two symbols" in msg
    import json
    v = json.loads(vocab)
    for key in (R.BOS, R.EOS):
        rc, msg = _create(json.dumps({k: i for k, i in v.items() if k != key}).encode(), b"")
        assert rc == -1 and f"the special token '{key}' is missing" in msg
    rc, msg = _create(b'{"a": 1, "b" 2}', b"")
    assert rc == -1 and "vocab.json: expected ':' at byte 13" in msg
    with pytest.raises(EdgeStyleHipError, match="cannot read"):
        NativeCLIPTokenizer(str(tmp_path / "nope.json"), full.mp)


def test_escaped_and_raw_vocabulary_files_load_alike(tmp_path):
    a = NativeCLIPTokenizer(*R.write_files(tmp_path / "esc", escape=True))
    b = NativeCLIPTokenizer(*R.write_files(tmp_path / "raw", escape=False))
    assert b"\\u" in open(a.vocab_file, "rb").read() and b"\\u" not in open(b.vocab_file, "rb").read()
    assert a.vocab_size == b.vocab_size == 2 * 256 + 2 + len(R.build_vocab()[1])
    texts = R.random_texts(50, seed=3)
    assert torch.equal(a(texts, **KW).input_ids, b(texts, **KW).input_ids)


# ---- the assembled prompt row -------------------------------------------------------------------------------------------------------
COLORS = DEFAULT_COLORS[:7]
ITEMS = DEFAULT_CLOTHING_ITEMS[:9]


def assemble_cases():
    """(name, nseg, k, topk [n, nseg, k]) - n = 3 rows each; -1, out-of-range and repeated entries included"""
    g = torch.Generator().manual_seed(8)
    out = []
    for nseg, sizes in ((1, [len(COLORS) + len(ITEMS)]), (2, [len(COLORS), len(ITEMS)])):
        for k in (1, 2, 8):
            t = torch.stack([torch.stack([torch.randint(0, s, (k,), generator=g) for s in sizes]) for _ in range(3)]).to(torch.int32)
            out.append((f"nseg{nseg}_k{k}", nseg, k, t))
            bad = t.clone()
            bad[0, 0, 0] = -1
            bad[1, nseg - 1, k - 1] = sizes[nseg - 1]                    # one past the segment
            bad[2, 0, k // 2] = 2 ** 31 - 1
            bad[2, nseg - 1, 0] = -2 ** 31
            if k == 8:
                bad[1, 0, :] = -1                                        # a whole segment empty
            out.append((f"nseg{nseg}_k{k}_bad", nseg, k, bad))
    return out


def joined(words, sizes, topk_row, prefix, sep, suffix, glue=" "):
    """the string whose tokenisation the assembled row must equal: the pieces joined by `glue`"""
    pieces, start = [prefix], 0
    for s, size in enumerate(sizes):
        for e in topk_row[s].tolist():
            if 0 <= e < size:
                pieces += [sep, words[start + e]]
        start += size
    return glue.join(pieces + [suffix])


@pytest.mark.parametrize("Lm", [8, 16, 77])
def test_assemble_host_equals_the_oracle_on_the_space_joined_string(tmp_path, Lm):
    c = Case(tmp_path / "t", holes=False, max_length=Lm)
    words = COLORS + ITEMS
    for suffix in ("", "best quality, a polo shirt they're wearing"):
        for name, nseg, k, topk in assemble_cases():
            sizes = [len(words)] if nseg == 1 else [len(COLORS), len(ITEMS)]
            seg_ends = [len(words)] if nseg == 1 else [len(COLORS), len(words)]
            table = c.native.prompt_table(words, seg_ends, prefix="edgestyle", separator=",", suffix=suffix)
            ids, eos = table.assemble_host(topk)
            texts = [joined(words, sizes, row, "edgestyle", ",", suffix) for row in topk]
            want = R.oracle_ids(c.oracle, texts, Lm)
            assert torch.equal(ids.to(torch.int64), want), (name, suffix, texts)
            totals = [len(c.oracle(t, add_special_tokens=False).input_ids) for t in texts]
            assert eos.tolist() == [1 + min(t, Lm - 2) for t in totals]
            table.close()
    # truncation inside a word happened at the short lengths: some row's last body id is not the last id of its last piece
    if Lm == 8:
        assert max(totals) > Lm - 2


def test_assemble_host_equals_the_comma_joined_reference_form(full):
    """the reference's string "edgestyle, c1, c2, i1, i2" + " " + suffix (and NativeBestEmbeddings.__call__'s) for the default lists"""
    from edgestyle_amd.clip import check_comma_join
    words = DEFAULT_COLORS + DEFAULT_CLOTHING_ITEMS
    check_comma_join(full.native, "edgestyle", words)
    g = torch.Generator().manual_seed(4)
    topk = torch.stack([torch.stack([torch.randperm(20, generator=g)[:2], torch.randperm(20, generator=g)[:2]]) for _ in range(30)]).to(torch.int32)
    for suffix in ("", "best quality, high resolution"):
        table = full.native.prompt_table(words, [20, 40], prefix="edgestyle", separator=",", suffix=suffix)
        ids, _ = table.assemble_host(topk)
        texts = ["edgestyle, " + ", ".join([DEFAULT_COLORS[int(j)] for j in row[0]] + [DEFAULT_CLOTHING_ITEMS[int(j)] for j in row[1]]) + " " + suffix
                 for row in topk]
        assert torch.equal(ids.to(torch.int64), R.oracle_ids(full.oracle, texts, 77))


def test_the_construction_check_names_the_word(full):
    from edgestyle_amd.clip import check_comma_join
    assert full.native.tokenize_ids("t-shirt!, x") != full.native.tokenize_ids("t-shirt! , x")      # why the check exists
    for word in ("shirt!", "coat)", "..."):
        with pytest.raises(EdgeStyleHipError, match="the word " + re.escape(repr(word)) + " tokenises differently"):
            check_comma_join(full.native, "edgestyle", ["red", word, "dress"])
    with pytest.raises(EdgeStyleHipError, match="the word 'edgestyle:'"):
        check_comma_join(full.native, "edgestyle:", ["red"])
    check_comma_join(full.native, "edgestyle", ["t-shirt", "tank top", "it's", "3", "(coat"])       # only the end meets the comma


def test_prompt_table_refusals(full):
    n = full.native
    with pytest.raises(EdgeStyleHipError, match="nseg must be in 1..4"):
        n.prompt_table(["a"] * 5, [1, 2, 3, 4, 5])
    with pytest.raises(EdgeStyleHipError, match="the last of seg_ends must be n_words"):
        n.prompt_table(["a", "b"], [1])
    with pytest.raises(EdgeStyleHipError, match="seg_ends must be increasing"):
        n.prompt_table(["a", "b"], [2, 2])
    with pytest.raises(EdgeStyleHipError, match=r"word 1: byte 0xC3 at offset 3"):
        n.prompt_table(["a", "café"], [2])
    with pytest.raises(EdgeStyleHipError, match=r"suffix: the text holds the special token literal"):
        n.prompt_table(["a"], [1], suffix="x <|endoftext|>")
    t = n.prompt_table(["a", "b"], [2])
    with pytest.raises(EdgeStyleHipError, match=r"k must be in 1\.\.8"):
        t.assemble_host(torch.zeros(1, 1, 9, dtype=torch.int32))
    lib, out = L.load(), (C.c_int32 * 77)()
    assert lib.es_prompt_assemble(t._h, C.c_void_p(0x1000), 1, 1, C.c_void_p(0x2000), None, None) == -1          # refused before any launch
    assert b"host memory alone" in lib.es_last_error()
    plan = lib.es_plan_create()
    try:
        assert lib.es_plan_begin_record(plan) == 0
        try:
            one = (C.c_int32 * 1)(0)
            assert lib.es_prompt_assemble_host(t._h, one, 1, 1, out, None) == -1 and b"never part of a plan" in lib.es_last_error()
            assert lib.es_text_encode_dev(C.c_void_p(0x1000), C.c_void_p(0x1000), 1, C.c_void_p(0x1000), None) == -1
            assert b"never part of a plan" in lib.es_last_error()
        finally:
            lib.es_plan_end_record(plan)
        assert lib.es_plan_size(plan) == 0
    finally:
        lib.es_plan_destroy(plan)


def test_native_tokenizer_inside_the_pipelines_clip_call(full):
    """pipeline._clip with tokenizer=NativeCLIPTokenizer hands the text encoder the oracle's input_ids"""
    from edgestyle_amd.pipeline import StableDiffusionControlNetPipeline
    seen = []

    class Encoder:
        def __call__(self, input_ids):
            seen.append(input_ids)
            return (torch.zeros(input_ids.shape[0], input_ids.shape[1], 4),)

    pipe = object.__new__(StableDiffusionControlNetPipeline)
    pipe.text_encoder = Encoder()
    texts = ["edgestyle, red, navy, dress, tank top best quality", ""]
    for tok in (full.native, full.oracle):
        pipe.tokenizer = tok
        pipe._clip(texts)
        pipe._clip(texts[0])
    assert torch.equal(seen[0], seen[2]) and torch.equal(seen[1], seen[3]) and seen[0].dtype == seen[2].dtype == torch.int64
    assert seen[1].shape == (1, 77)


def test_cli_flag_is_off_by_default():
    from edgestyle_amd.cli import parse_args
    assert parse_args([]).native_tokenizer is False
    assert parse_args(["--native_tokenizer"]).native_tokenizer is True
