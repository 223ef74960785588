#!/usr/bin/env python
"""The bits the five encoder-stack handles compute, as SHA-256 lines: run it on two builds and compare the outputs line for line.

Only the public Python API is used (NativeCondEncoder, NativeDetokenizer, NativeAudioTokenizer.pool, NativeTextEncoder, NativeCausalLM
prefill / decode), so the same file runs on any build.  Weights and inputs are seeded and generated on the CPU; every handle is tiny (256
wide, two layers).  Each handle runs a small call, a larger one that makes its workspace grow, and the small one again:

  * condition encoder: two items with lyric lengths (70, 0) and text lengths (9, 0) - a full and an empty one -, three reference clips;
    then 130 lyric rows and clips of 70; then the first call again
  * detokenizer and tokenizer: 2 x 7 windows, 3 x 40, 2 x 7
  * text encoder: 2 sequences of S = 1, 64, 65, 130, then 64 again
  * LM: prefills of P = 1, 17, 64, 65, 130 with left padding (first = 0, 5, P - 1); then a prefill of 250 columns and twelve decode steps,
    which cross the decode plan's boundary 256 | 257
Usage: python tools/encoder_bits.py [--out FILE] [--root DIR]     (DIR: the checkout to import, default this file's)
"""
from __future__ import annotations

import argparse
import hashlib
import os
import sys

TINY = dict(hidden_size=256, intermediate_size=768, num_attention_heads=2, num_key_value_heads=1, head_dim=128)


def run(root):
    sys.path.insert(0, root)
    import torch
    import ace355
    from ace355 import weightgen
    from ace355.cond import NativeCondEncoder
    from ace355.config import LmConfig, TextEncoderConfig
    from ace355.lm import NativeCausalLM
    from ace355.lmhints import NativeAudioTokenizer, NativeDetokenizer
    from ace355.textenc import NativeTextEncoder

    lines = []

    def say(what, t):
        ln = f"{what} {hashlib.sha256(t.contiguous().cpu().view(torch.int32).numpy().tobytes()).hexdigest()}"
        print(ln, flush=True)
        lines.append(ln)

    def rnd(seed, *shape):
        return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))

    def gen(shapes, seed):
        return weightgen.make_dit_weights(shapes, 256, seed=seed, mode="test")

    def prefix_mask(L, lens):
        return (torch.arange(L)[None] < torch.tensor(lens)[:, None]).long()

    # ---- condition encoder
    ccfg = ace355.CondConfig(**TINY, text_hidden_dim=64, timbre_hidden_dim=64, num_lyric_encoder_hidden_layers=2, num_timbre_encoder_hidden_layers=2,
                             sliding_window=16)
    cond = NativeCondEncoder(ccfg, "cuda:0")
    cond.load_state_dict(gen(ccfg.weight_shapes(), 31))
    order = torch.tensor([0, 1, 1])
    for tag, Ll, Tref in (("small", 70, 33), ("large", 130, 70), ("small again", 70, 33)):
        out, mask = cond(rnd(1, 2, 9, 64), prefix_mask(9, [9, 0]), rnd(2, 2, Ll, 64), prefix_mask(Ll, [Ll, 0]), rnd(3, 3, Tref, 64), order)
        say(f"cond {tag} hidden", out.float())
        say(f"cond {tag} mask", mask.to(torch.int32))
    cond.close()

    # ---- detokenizer, tokenizer
    dcfg = ace355.DetokConfig(**TINY)
    detok = NativeDetokenizer(dcfg, "cuda:0")
    detok.load_state_dict(gen(dcfg.weight_shapes(), 32))
    for tag, B, T5 in (("small", 2, 7), ("large", 3, 40), ("small again", 2, 7)):
        say(f"detok {tag}", detok(rnd(4, B, T5, 256)).float())
    detok.close()
    D = dcfg.hidden_size
    tshapes = {"audio_acoustic_proj.weight": (D, dcfg.audio_acoustic_hidden_dim), "audio_acoustic_proj.bias": (D,),
               "attention_pooler.embed_tokens.weight": (D, D), "attention_pooler.embed_tokens.bias": (D,), "attention_pooler.norm.weight": (D,),
               "attention_pooler.special_token": (1, 1, D),
               **{"attention_pooler." + k: v for k, v in dcfg.weight_shapes().items() if k.startswith("layers.")}}
    tok = NativeAudioTokenizer(dcfg, "cuda:0")
    tok.load_state_dict(gen(tshapes, 33))
    for tag, B, T5 in (("small", 2, 7), ("large", 3, 40), ("small again", 2, 7)):
        say(f"tok {tag}", tok.pool(rnd(5, B, T5 * dcfg.pool_window_size, dcfg.audio_acoustic_hidden_dim)).float())
    tok.close()

    # ---- text encoder
    tcfg = TextEncoderConfig(**TINY, num_hidden_layers=2, vocab_size=515)
    te = NativeTextEncoder(tcfg, "cuda:0")
    te.load_state_dict(gen(tcfg.weight_shapes(), 34))
    for S in (1, 64, 65, 130, 64):
        ids = torch.randint(0, tcfg.vocab_size, (2, S), generator=torch.Generator().manual_seed(40 + S))
        say(f"textenc S = {S}", te(ids).last_hidden_state.view(torch.int16).to(torch.int32))
    te.close()

    # ---- LM
    lcfg = LmConfig(**TINY, num_hidden_layers=2, vocab_size=515, tie_word_embeddings=True)
    lm = NativeCausalLM(lcfg, "cuda:0", max_positions=300, max_seqs=4)
    lm.load_state_dict(gen(lcfg.weight_shapes(), 35))

    def left_padded(P, first, seed):
        ids = torch.randint(0, lcfg.vocab_size, (len(first), P), generator=torch.Generator().manual_seed(seed))
        mask = (torch.arange(P)[None] >= torch.tensor(first)[:, None]).long()
        return ids * mask, mask

    for P in (1, 17, 64, 65, 130):
        ids, mask = left_padded(P, [min(f, P - 1) for f in (0, 5, P - 1)], 50 + P)
        say(f"lm prefill P = {P}", lm.prefill(ids, mask))
    ids, mask = left_padded(250, [0, 5, 200], 60)
    say("lm prefill P = 250", lm.prefill(ids, mask))
    nxt = torch.randint(0, lcfg.vocab_size, (3, 12), generator=torch.Generator().manual_seed(61))
    for t in range(12):
        say(f"lm decode to length {251 + t}", lm.decode(nxt[:, t]))
    lm.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    lines = run(args.root)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
