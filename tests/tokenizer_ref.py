"""A seeded synthetic CLIP vocabulary and the oracle of the tokenizer tests: transformers' CLIPTokenizer built from the same two files.

The vocabulary is the 256-symbol byte-level alphabet, every symbol's </w> form, the merges a plain BPE trainer learns from the small
corpus below (so they are real: multi-level, overlapping, some ending a word and some not) and the two special tokens.  `holes=True`
takes some letters and some </w> forms out again (with every merge that needs them): the unk path."""
import collections
import json
import os
import random

from edgestyle_amd.prompts import DEFAULT_CLOTHING_ITEMS, DEFAULT_COLORS

N_MERGES = 60
BOS, EOS = "<|startoftext|>", "<|endoftext|>"
# the bytes the native tokenizer accepts
ACCEPTED = bytes(list(range(0x09, 0x0E)) + list(range(0x20, 0x7F)))
CORPUS = """edgestyle, a photo of a person wearing a shirt and the trousers, best quality, high resolution
the model is standing in the street, she's wearing a red dress, it's the best dress, they're wearing shorts
a t-shirt, a polo shirt and a tank top, that isn't a sweater, we've seen the jacket, i'll wear the hoodie, he'd wear jeans
there are 12 shirts and 345 dresses in the shop... really?! yes!!! (no) [maybe] 100% 3.50 10-20
low quality, worst quality, blurry, bad anatomy, bad hands, the the the and and wearing wearing shirt shirt dress dress
""" + " ".join(DEFAULT_COLORS * 3 + DEFAULT_CLOTHING_ITEMS * 3)
HOLES = ["q", "z", "k", "x</w>", "e</w>", "!</w>", ",", "7", "7</w>", "'</w>"]


def bytes_to_unicode():
    """the byte-level alphabet (GPT-2's): printable bytes stand for themselves, the others move up past 255"""
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAD)) + list(range(0xAE, 0x100))
    cs = bs[:]
    n = 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return {b: chr(c) for b, c in zip(bs, cs)}


def _pre_tokens(text):
    """enough of the split for a training corpus: lowercase, runs of letters, single digits, runs of the rest"""
    out, cur, kind = [], "", None
    for ch in text.lower():
        k = "s" if ch.isspace() else "l" if ch.isalpha() else "d" if ch.isdigit() else "p"
        if k != kind or k == "d":
            if cur and kind != "s":
                out.append(cur)
            cur = ""
        cur, kind = cur + ch, k
    if cur and kind != "s":
        out.append(cur)
    return out


def learn_merges(corpus, n):
    words = collections.Counter(tuple(w[:-1]) + (w[-1] + "</w>",) for w in _pre_tokens(corpus))
    merges = []
    for _ in range(n):
        pairs = collections.Counter()
        for w, c in words.items():
            for a, b in zip(w, w[1:]):
                pairs[(a, b)] += c
        if not pairs:
            break
        best = max(sorted(pairs), key=lambda p: pairs[p])
        merges.append(best)
        new = collections.Counter()
        for w, c in words.items():
            o, i = [], 0
            while i < len(w):
                if i + 1 < len(w) and (w[i], w[i + 1]) == best:
                    o.append(w[i] + w[i + 1])
                    i += 2
                else:
                    o.append(w[i])
                    i += 1
            new[tuple(o)] += c
        words = new
    return merges


def build_vocab(holes=False, seed=0):
    """(vocab dict, merges list): ids are shuffled by the seed, so nothing depends on their order"""
    alphabet = list(bytes_to_unicode().values())
    tokens = alphabet + [a + "</w>" for a in alphabet]
    merges = learn_merges(CORPUS, N_MERGES)
    if holes:
        gone = set(HOLES)
        tokens = [t for t in tokens if t not in gone]
        have, kept = set(tokens), []
        for a, b in merges:                    # a merge survives when both parts do (its result is then added)
            if a in have and b in have:
                kept.append((a, b))
                have.add(a + b)
        merges = kept
    tokens += [a + b for a, b in merges if a + b not in tokens]
    tokens += [BOS, EOS]
    assert len(set(tokens)) == len(tokens)
    order = list(range(len(tokens)))
    random.Random(seed).shuffle(order)
    return {t: i for t, i in zip(tokens, order)}, merges


def write_files(directory, holes=False, seed=0, escape=True):
    """vocab.json (escape: \\uXXXX keys, as transformers saves them; else raw UTF-8) and merges.txt -> their paths"""
    vocab, merges = build_vocab(holes, seed)
    os.makedirs(str(directory), exist_ok=True)
    vp, mp = os.path.join(str(directory), "vocab.json"), os.path.join(str(directory), "merges.txt")
    with open(vp, "w", encoding="utf-8") as f:
        json.dump(vocab, f, ensure_ascii=escape)
    with open(mp, "w", encoding="utf-8") as f:
        f.write("#version: 0.2\n" + "".join(f"{a} {b}\n" for a, b in merges))
    return vp, mp


def oracle(vocab_path, merges_path, max_length=77):
    from transformers import CLIPTokenizer
    return CLIPTokenizer(vocab_path, merges_path, model_max_length=max_length)


def oracle_ids(tok, texts, max_length):
    return tok(list(texts), padding="max_length", max_length=max_length, truncation=True, return_tensors="pt").input_ids


def random_texts(n, seed, max_len=300):
    """strings of length 0..max_len over the accepted bytes only; white space and the apostrophe forms come up often enough to matter"""
    rng = random.Random(seed)
    pool = [chr(b) for b in ACCEPTED]
    heavy = [" ", " ", " ", "\t", "\n", "'s", "'t", "'re", "'ve", "'m", "'ll", "'d", "'", "e", "t", "a", "s", "r", "S", "T", ",", ".", "!", "7", "0"]
    words = DEFAULT_COLORS + DEFAULT_CLOTHING_ITEMS + ["wearing", "the", "Shirt", "DRESS", "it's", "they're"]
    out = []
    for _ in range(n):
        target, s = rng.randint(0, max_len), ""
        while len(s) < target:
            r = rng.random()
            s += rng.choice(pool) if r < 0.45 else rng.choice(heavy) if r < 0.8 else rng.choice(words)
        out.append(s[:target])
    return out
