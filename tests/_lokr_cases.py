"""LoKr merge: the tiny cases the GPU tests run, the exactness gate they apply, and an fp32 emulation of the contract with seedable
defects (tests/test_lokr_gpu.py applies the gate to the kernel, tests/test_lokr_cpu.py proves the gate on the emulation).

Contract (include/ace355.h ``ace355_dit_set_adapters_mixed``): got = bf16_rne(float(W0) + sum_j s_j kron(W1_j, W2_j)), a decomposed
factor's product a @ b and every other product and sum in fp32, the terms in call order, one rounding.

Gate, derived and not measured.  fp32 work per element and term: r dependent roundings for a rank-r factor product (r products summed
in r - 1 additions, bounded by r), the scale, the Kronecker product and the addition to the running sum = r1 + r2 + 3; the addition
to W0 once.  With u = 2^-24, mag = |W0| + sum |s| (|w1_a| |w1_b|) kron (|w2_a| |w2_b|) and E = (1 + sum_terms (r1 + r2 + 3)) u mag the
fp32 value the kernel rounds lies within E of the exact one, so for every element
    |got - exact| <= ulp / 2 + E                      (ulp: the bf16 spacing at |exact| + E)
    got == bf16_rne(exact)  wherever exact is further than E from a bf16 rounding tie,
and the share of elements within E of a tie is capped (2 % at the tiny shapes, 5 % at full size): inputs whose sum cancels so far
that E reaches the rounding step would make the second bound vacuous.
"""
import torch

TINY = dict(hidden_size=256, intermediate_size=768, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1, head_dim=128)
KINDS = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "cross_attn.q_proj", "cross_attn.k_proj",
         "cross_attn.v_proj", "cross_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")
# one target per weight shape of the tiny configuration: 256 x 256, 128 x 256, 768 x 256, 256 x 768
SHAPE_TARGETS = ("layers.0.self_attn.q_proj.weight", "layers.0.cross_attn.k_proj.weight", "layers.0.mlp.up_proj.weight",
                 "layers.0.mlp.down_proj.weight")
# (out_l, in_m, r1, r2); "full" = (out, in, 0, 0): W2 is 1 x 1
SPLITS = ((16, 16, 0, 0), (16, 64, 0, 8), (8, 32, 4, 40), (24, 16, 0, 1), (2, 3, 0, 64), (1, 1, 0, 8), "full")


def bf(x):
    return x.to(torch.bfloat16).float()


def make_term(name, shape, split, gen, rel_size=0.5, w0=None):
    """A seeded KronTerm for ``name`` [out, in] with bf16-held factors: unit-normal factors, the b factors scaled by r^-1/2; the scale
    makes ||s kron(W1, W2)|| = rel_size x ||W0||."""
    from ace355.lokr import KronTerm, dense_delta
    out_f, in_f = shape
    out_l, in_m, r1, r2 = (out_f, in_f, 0, 0) if split == "full" else split
    assert out_f % out_l == 0 and in_f % in_m == 0, (name, shape, split)
    out_k, in_n = out_f // out_l, in_f // in_m

    def factor(rows, cols, r):
        if r == 0:
            return bf(torch.randn(rows, cols, generator=gen)), None, None
        return None, bf(torch.randn(rows, r, generator=gen)), bf(torch.randn(r, cols, generator=gen) * r ** -0.5)
    w1, w1a, w1b = factor(out_l, in_m, r1)
    w2, w2a, w2b = factor(out_k, in_n, r2)
    t = KronTerm(name, w1, w1a, w1b, w2, w2a, w2b, 1.0)
    s = 1.0 if w0 is None else rel_size * float(w0.norm()) / float(dense_delta(t).norm())
    return t._replace(scale=s)


def split_fits(shape, split):
    return split == "full" or (shape[0] % split[0] == 0 and shape[1] % split[1] == 0)


def tiny_cases(cfg, w):
    """[(label, [terms of one set_adapters call])]: every split on every target shape it divides, the two-term case at a relative size
    of 3, and all ten kinds of both layers in one call."""
    shapes = cfg.weight_shapes()
    cases = []
    for si, split in enumerate(SPLITS):
        g = torch.Generator().manual_seed(100 + si)
        terms = [make_term(n, shapes[n], split, g, w0=w[n]) for n in SHAPE_TARGETS if split_fits(shapes[n], split)]
        assert terms, split
        cases.append((f"split {split}", terms))
    g = torch.Generator().manual_seed(200)
    n = SHAPE_TARGETS[2]
    cases.append(("two terms on one target, relative size 3",
                  [make_term(n, shapes[n], (8, 32, 4, 8), g, rel_size=3.0, w0=w[n]), make_term(n, shapes[n], (24, 16, 0, 1), g, rel_size=3.0, w0=w[n]),
                   make_term(SHAPE_TARGETS[0], shapes[SHAPE_TARGETS[0]], (16, 16, 0, 0), g, rel_size=3.0, w0=w[SHAPE_TARGETS[0]]),
                   make_term(SHAPE_TARGETS[0], shapes[SHAPE_TARGETS[0]], (16, 64, 0, 8), g, rel_size=3.0, w0=w[SHAPE_TARGETS[0]])]))
    cases.append(("all ten kinds, both layers", all_kinds_terms(cfg, w, seed=300)))
    return cases


def all_kinds_terms(cfg, w, seed, rel_size=0.5, split=(8, 8, 0, 8)):
    g = torch.Generator().manual_seed(seed)
    shapes = cfg.weight_shapes()
    return [make_term(f"layers.{li}.{k}.weight", shapes[f"layers.{li}.{k}.weight"], split, g, rel_size=rel_size, w0=w[f"layers.{li}.{k}.weight"])
            for li in range(cfg.num_hidden_layers) for k in KINDS]


def merged(w, terms):
    """The fp32 dict w0 + sum s kron(W1, W2) (the oracle's expectation)."""
    from ace355.lokr import dense_delta
    m = dict(w)
    for t in terms:
        m[t.name] = (m[t.name].double() + dense_delta(t)).float()
    return m


# ---------------------------------------------------------------- the gate
def _factor64(w, a, b, dev):
    if w is not None:
        x = w.double().to(dev)
        return x, x.abs(), 0
    a, b = a.double().to(dev), b.double().to(dev)
    return a @ b, a.abs() @ b.abs(), a.shape[1]


def bounds(w0_bf16, terms):
    """(exact float64, E) of one target from its bf16 base and its terms (factors as the kernel holds them: bf16 values)."""
    w0 = w0_bf16.double()
    dev = w0.device
    exact, mag, ops = w0.clone(), w0.abs(), 1
    for t in terms:
        w1, a1, r1 = _factor64(t.w1, t.w1_a, t.w1_b, dev)
        w2, a2, r2 = _factor64(t.w2, t.w2_a, t.w2_b, dev)
        s = float(torch.tensor(t.scale, dtype=torch.float32))   # (the C ABI carries the scale as a float)
        exact += s * torch.kron(w1, w2)
        mag += abs(s) * torch.kron(a1, a2)
        ops += r1 + r2 + 3
    return exact, ops * 2.0 ** -24 * mag


def _ulp(x):
    return torch.exp2(torch.floor(torch.log2(x.clamp_min(2.0 ** -126))) - 7)


def gate(got_bf16, w0_bf16, terms, what, tie_cap=0.02):
    """Assert both bounds and the cap; returns (share of elements bit-equal to bf16_rne(exact), share within E of a tie, worst
    |got - exact| - ulp / 2 in units of E)."""
    exact, E = bounds(w0_bf16, terms)
    got = got_bf16.to(exact.device).double()
    err = (got - exact).abs()
    half = 0.5 * _ulp(exact.abs() + E)
    worst = float(((err - half) / E.clamp_min(1e-300)).max())
    frac = exact.abs() / _ulp(exact.abs())          # in units of the bf16 spacing: ties sit at k + 1/2
    tie_dist = ((frac - torch.floor(frac)) - 0.5).abs() * _ulp(exact.abs())
    near = tie_dist <= E
    exp = exact.to(torch.bfloat16).double()
    same = got == exp
    share_near = float(near.double().mean())
    wrong_far = int((~same & ~near).sum())
    print(f"    [lokr gate] {what}: {100 * float(same.double().mean()):.3f} % bit-equal to bf16_rne(float64), {100 * share_near:.3f} % within E of a "
          f"tie (cap {100 * tie_cap:.0f} %), {wrong_far} mismatches outside that set, worst (|err| - ulp/2) / E = {worst:.3f}")
    assert share_near <= tie_cap, (what, "share of elements within E of a tie", share_near)
    assert worst <= 1.0, (what, "|got - exact| > ulp / 2 + E", worst)
    assert wrong_far == 0, (what, "got != bf16_rne(exact) away from every tie", wrong_far)
    return float(same.double().mean()), share_near, worst


# ---------------------------------------------------------------- fp32 emulation of the contract, with seedable defects
DEFECTS = ("swap_kl", "in_n_stride", "drop_second_term", "scale_twice", "bf16_w2", "corrupt_group")


def emulate(w0_bf16, terms, defect=None):
    """The contract in fp32 on the CPU: bf16 result of one target.  ``defect`` seeds one of DEFECTS."""
    assert defect is None or defect in DEFECTS
    out_f, in_f = w0_bf16.shape
    total = torch.zeros(out_f, in_f, dtype=torch.float32)
    rows, cols = torch.arange(out_f), torch.arange(in_f)
    first = None
    for j, t in enumerate(terms):
        if defect == "drop_second_term" and j == 1:
            continue
        w1 = t.w1.float() if t.w1 is not None else t.w1_a.float() @ t.w1_b.float()
        w2 = t.w2.float() if t.w2 is not None else t.w2_a.float() @ t.w2_b.float()
        if defect == "bf16_w2":
            w2 = bf(w2)
        (out_l, in_m), (out_k, in_n) = w1.shape, w2.shape
        s = torch.tensor(t.scale, dtype=torch.float32)
        if defect == "scale_twice":
            s = s * s
        l, k, m, n = rows // out_k, rows % out_k, cols // in_n, cols % in_n
        if defect == "swap_kl":   # row = k out_l + l instead of l out_k + k
            l, k = rows % out_l, rows // out_l
        if defect == "in_n_stride":   # column = m (in_n + 1) + n
            m = (cols // (in_n + 1)).clamp_max(in_m - 1)
        d = (s * w1)[l][:, m] * w2[k][:, n]
        if first is None:
            first = (t, l, k, m, n, s, w1, w2)
        total = total + d
    got = (w0_bf16.float() + total).to(torch.bfloat16)
    if defect == "corrupt_group":   # one 8-column group at an m boundary takes W1 of the previous m
        t, l, k, m, n, s, w1, w2 = first
        in_n = w2.shape[1]
        c = min(in_n // 8 * 8, in_f - 8)   # the group that holds the first m boundary
        r = out_f // 2
        mm = (m[c:c + 8] - 1).clamp_min(0) if w1.shape[1] > 1 else m[c:c + 8]
        bad = (s * w1)[l[r]][mm] * w2[k[r]][n[c:c + 8]]
        if w1.shape[1] == 1:
            bad = bad * 1.5
        wrong = total[r, c:c + 8] - ((s * w1)[l[r]][m[c:c + 8]] * w2[k[r]][n[c:c + 8]]) + bad
        got[r, c:c + 8] = (w0_bf16[r, c:c + 8].float() + wrong).to(torch.bfloat16)
    return got


def by_target(terms):
    out = {}
    for t in terms:
        out.setdefault(t.name, []).append(t)
    return out
