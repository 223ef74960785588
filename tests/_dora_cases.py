"""DoRA merge: the tiny cases the GPU tests run, the exactness gate they apply, and an fp32 emulation of the contract with seedable
defects (tests/test_dora_gpu.py applies the gate to the kernel, tests/test_dora_cpu.py proves the gate on the emulation).

Contract (include/ace355.h ``ace355_dit_set_adapters_dora``): with V the fp32 value the plain merge rounds,
    n = ||V||_2 along the row (axis "out") or the column (axis "in"), from an fp64 sum of the squares of the fp32 V,
    f = fp32(1 + m (g / (n + eps) - 1)) formed in fp64,        got = bf16_rne(fp32(V f)).

Gate, derived and not measured.  Let Ev be the bound on |V^ - V| of the plain merge: ``_lokr_cases.bounds`` for Kronecker terms; for
LoRA terms (1 + sum_terms (2 r + 2)) u mag with u = 2^-24 and mag = |W0| + sum |s| |B| |A| - r accumulation steps inside the MFMA,
each allowed 2 u of the running magnitude (an internal addition that truncates is covered), the scale, the addition to the running sum,
and the addition to W0 once.  Then
  * the norm moves by at most En = ||Ev||_2 along the axis (the triangle inequality; the fp64 reduction itself adds less than
    1e-12 n, which is added),
  * f(n) = 1 - m + m g / (n + eps) is a hyperbola in n, so |f(n^) - f(n)| <= |m g| En / ((n + eps)(n + eps - En)) =: Df, and the single
    fp32 rounding of f adds u (|f| + Df): Ef = Df + u (|f| + Df),
  * the product: |V^ f^ - V f| <= Ev (|f| + Ef) + |V| Ef, and its fp32 rounding adds u (|V| + Ev)(|f| + Ef).
E is the sum of the last line.  The three assertions are those of ``_lokr_cases.gate``: |got - exact| <= ulp / 2 + E, got ==
bf16_rne(exact) wherever exact is further than E from a rounding tie, and at most 2 % (tiny) / 5 % (full size) of the elements within
E of a tie.
"""
import torch

import _lokr_cases as L

TINY, KINDS, SHAPE_TARGETS = L.TINY, L.KINDS, L.SHAPE_TARGETS
# the additive parts: LoKr splits (the rank-40 split of the LoKr cases sits at 1.7 - 1.9 % within E of a tie, too close to the cap)
SPLITS = ((16, 16, 0, 0), (16, 64, 0, 8), (24, 16, 0, 1), "full")
LORA_RANK = 8
EPS_BF16 = 2.0 ** -7
U = 2.0 ** -24
# packed row layouts of the targets (csrc/common.h pack_row): q / k of both attentions HEADPAIR, gate / up IL32, the rest plain
HEADPAIR_KINDS = ("self_attn.q_proj", "self_attn.k_proj", "cross_attn.q_proj", "cross_attn.k_proj")
IL32_KINDS = ("mlp.gate_proj", "mlp.up_proj")


def bf(x):
    return x.to(torch.bfloat16).float()


def is_dora(t):
    return hasattr(t, "per_input")


def is_kron(t):
    return hasattr(t, "w1_a")


def split_terms(terms):
    """(additive terms by target, DoraTerm by target) of one set_adapters call."""
    add, dora = {}, {}
    for t in terms:
        if is_dora(t):
            assert t.name not in dora
            dora[t.name] = t
        else:
            add.setdefault(t.name, []).append(t)
    return add, dora


def make_lora(name, shape, gen, w0, rank=LORA_RANK, rel_size=0.5):
    from ace355.lora import LoraTerm
    o, i = shape
    A, B = bf(torch.randn(rank, i, generator=gen)), bf(torch.randn(o, rank, generator=gen))
    return LoraTerm(name, A, B, rel_size * float(w0.norm()) / float((B @ A).norm()))


def additive_bounds(w0_bf16, terms):
    """(exact V float64, Ev) of one target from its bf16 base and its additive terms (all Kronecker or all LoRA)."""
    if not terms or is_kron(terms[0]):
        assert all(is_kron(t) for t in terms)
        return L.bounds(w0_bf16, terms)
    w0 = w0_bf16.double()
    dev = w0.device
    exact, mag, ops = w0.clone(), w0.abs(), 1
    for t in terms:
        B, A = t.B.double().to(dev), t.A.double().to(dev)
        s = float(torch.tensor(t.scale, dtype=torch.float32))
        exact += s * (B @ A)
        mag += abs(s) * (B.abs() @ A.abs())
        ops += 2 * A.shape[0] + 2
    return exact, ops * U * mag


def _f64(v, d):
    """(n, f) in float64 along the axis of the DoraTerm ``d`` for the merged ``v`` (float64), broadcastable against v."""
    dim = 0 if d.per_input else 1
    g = d.g.detach().float().double().reshape(-1).to(v.device)
    g = g[None, :] if d.per_input else g[:, None]
    n = v.norm(dim=dim, keepdim=True)
    m, eps = float(torch.tensor(d.scale, dtype=torch.float32)), float(torch.tensor(d.eps, dtype=torch.float32))
    den = n + eps
    f = torch.where(den == 0, torch.ones_like(den), 1 + m * (g / den.clamp_min(1e-300) - 1))
    return n, f, g, m, eps


def dense(w0_bf16, terms, d):
    """The float64 DoRA merge of one target."""
    v, _ = additive_bounds(w0_bf16, terms)
    return v * _f64(v, d)[1]


def bounds(w0_bf16, terms, d):
    """(exact float64, E) of one target under the DoraTerm ``d`` (module docstring)."""
    v, ev = additive_bounds(w0_bf16, terms)
    n, f, g, m, eps = _f64(v, d)
    en = ev.norm(dim=0 if d.per_input else 1, keepdim=True) + 1e-12 * n
    den = n + eps
    assert bool((den > 2 * en).all()), "a row / column whose norm is within its own error bound: the gate says nothing there"
    df = (m * g).abs() * en / (den * (den - en))
    ef = df + U * (f.abs() + df)
    e = ev * (f.abs() + ef) + v.abs() * ef + U * (v.abs() + ev) * (f.abs() + ef)
    return v * f, e


def gate(got_bf16, w0_bf16, terms, d, what, tie_cap=0.02):
    """The three assertions of ``_lokr_cases.gate`` with the DoRA ``exact`` and ``E``; returns (share bit-equal to bf16_rne(exact),
    share within E of a tie, worst (|got - exact| - ulp / 2) / E)."""
    exact, E = bounds(w0_bf16, terms, d)
    got = got_bf16.to(exact.device).double()
    err = (got - exact).abs()
    half = 0.5 * L._ulp(exact.abs() + E)
    worst = float(((err - half) / E.clamp_min(1e-300)).max())
    frac = exact.abs() / L._ulp(exact.abs())
    tie_dist = ((frac - torch.floor(frac)) - 0.5).abs() * L._ulp(exact.abs())
    near = tie_dist <= E
    same = got == exact.to(torch.bfloat16).double()
    share_near = float(near.double().mean())
    wrong_far = int((~same & ~near).sum())
    print(f"    [dora gate] {what}: {100 * float(same.double().mean()):.3f} % bit-equal to bf16_rne(float64), {100 * share_near:.3f} % within E "
          f"of a tie (cap {100 * tie_cap:.0f} %), {wrong_far} mismatches outside that set, worst (|err| - ulp/2) / E = {worst:.3f}")
    assert share_near <= tie_cap, (what, "share of elements within E of a tie", share_near)
    assert worst <= 1.0, (what, "|got - exact| > ulp / 2 + E", worst)
    assert wrong_far == 0, (what, "got != bf16_rne(exact) away from every tie", wrong_far)
    return float(same.double().mean()), share_near, worst


def make_dora(name, w0_bf16, terms, per_input, m, eps, gen):
    """g = bf16(n_exact (1 + 0.25 randn)): the factor moves the elements by many bf16 steps."""
    from ace355.dora import DoraTerm
    v, _ = additive_bounds(w0_bf16, terms)
    n = v.norm(dim=0 if per_input else 1).cpu()
    g = (n * (1 + 0.25 * torch.randn(n.shape, generator=gen).double())).to(torch.bfloat16)
    return DoraTerm(name, g, bool(per_input), float(eps), float(m))


def _additive(kind, names, shapes, w, gen):
    if kind == "lora":
        return [make_lora(n, shapes[n], gen, w[n]) for n in names]
    return [L.make_term(n, shapes[n], kind, gen, w0=w[n]) for n in names if L.split_fits(shapes[n], kind)]


def tiny_cases(cfg, w):
    """[(label, [terms of one set_adapters call])]: every additive kind (four LoKr splits, rank-8 LoRA) on every target shape it
    divides x both axes x two of the four (m, eps) pairs (all four occur on both axes), all ten kinds of both layers in one call, and a
    call in which only some targets carry DoRA (both additive families, so both merge kernels run plain and decomposed at once)."""
    shapes = cfg.weight_shapes()
    w0 = {n: w[n].to(torch.bfloat16) for n in shapes if n.startswith("layers.") and n.endswith("_proj.weight")}
    cases = []
    for ki, kind in enumerate(SPLITS + ("lora",)):
        for per_input in (False, True):
            pairs = ((1.0, EPS_BF16), (0.6, 0.0)) if (ki + per_input) % 2 == 0 else ((1.0, 0.0), (0.6, EPS_BF16))
            for m, eps in pairs:
                g = torch.Generator().manual_seed(1000 + 8 * ki + 4 * per_input + 2 * (m != 1.0) + (eps != 0.0))
                add = _additive(kind, SHAPE_TARGETS, shapes, w, g)
                assert add, kind
                dora = [make_dora(t.name, w0[t.name], [t], per_input, m, eps, g) for t in add]
                cases.append((f"{kind}, axis {'in' if per_input else 'out'}, m {m}, eps {eps}", add + dora))
    g = torch.Generator().manual_seed(2000)
    add = L.all_kinds_terms(cfg, w, seed=2001)
    cases.append(("all ten kinds, both layers",
                  add + [make_dora(t.name, w0[t.name], [t], i % 2 == 1, (1.0, 0.6)[i % 3 == 0], (EPS_BF16, 0.0)[i % 5 == 0], g)
                         for i, t in enumerate(add)]))
    g = torch.Generator().manual_seed(2100)
    names = [f"layers.{li}.{k}.weight" for li in range(cfg.num_hidden_layers) for k in KINDS]
    add = [L.make_term(n, shapes[n], (8, 8, 0, 8), g, w0=w[n]) if i % 2 else make_lora(n, shapes[n], g, w[n]) for i, n in enumerate(names)]
    cases.append(("DoRA on some targets only, both families",
                  add + [make_dora(t.name, w0[t.name], [t], i % 4 == 0, 1.0, EPS_BF16, g) for i, t in enumerate(add) if i % 3 != 2]))
    return cases


def merged(w, terms):
    """The fp32 dict of the float64 merge, DoRA included (the oracle's expectation)."""
    add, dora = split_terms(terms)
    m = dict(w)
    for name, ts in add.items():
        w0 = w[name].to(torch.bfloat16)
        m[name] = (dense(w0, ts, dora[name]) if name in dora else additive_bounds(w0, ts)[0]).float()
    return m


# ---------------------------------------------------------------- fp32 emulation of the contract, with seedable defects
DEFECTS = ("swap_axis", "drop_eps", "drop_m", "norm_of_w0", "own_tile_only", "g_by_packed_row", "fp32_accumulation")
TILE_ROWS, TILE_COLS = 64, 128


def packed_row(name, r):
    """Packed row of reference row ``r`` (a tensor) inside the target's own block of rows (csrc/common.h pack_row without row0)."""
    if any(k in name for k in IL32_KINDS):
        return (r // 32) * 64 + (r % 32)   # (the gate | up interleave: 32 rows of one, 32 of the other)
    if any(k in name for k in HEADPAIR_KINDS):
        d = r % 128
        return (r - d) + torch.where(d < 64, 2 * d, 2 * (d - 64) + 1)
    return r


def v32(w0_bf16, terms):
    """The fp32 V of the plain merge: fp32 products and sums, the terms in call order."""
    out_f, in_f = w0_bf16.shape
    total = torch.zeros(out_f, in_f, dtype=torch.float32)
    rows, cols = torch.arange(out_f), torch.arange(in_f)
    for t in terms:
        s = torch.tensor(t.scale, dtype=torch.float32)
        if is_kron(t):
            w1 = t.w1.float() if t.w1 is not None else t.w1_a.float() @ t.w1_b.float()
            w2 = t.w2.float() if t.w2 is not None else t.w2_a.float() @ t.w2_b.float()
            out_k, in_n = w2.shape
            total = total + (s * w1)[rows // out_k][:, cols // in_n] * w2[rows % out_k][:, cols % in_n]
        else:
            total = total + s * (t.B.float() @ t.A.float())
    return w0_bf16.float() + total


def emulate(w0_bf16, terms, d, defect=None):
    """The contract on the CPU: bf16 result of one target.  ``defect`` seeds one of DEFECTS."""
    assert defect is None or defect in DEFECTS
    v = v32(w0_bf16, terms)
    out_f, in_f = v.shape
    per_input = bool(d.per_input)
    src = w0_bf16.float() if defect == "norm_of_w0" else v
    dim = 0 if per_input else 1
    if defect == "swap_axis":   # the norm along the other axis, read at the index of this one
        other = src.double().pow(2).sum(dim=1 - dim).sqrt()
        n = other[torch.arange(in_f if per_input else out_f) % other.numel()]
        n = n[None, :] if per_input else n[:, None]
    elif defect == "own_tile_only":   # the partials of the other tiles are never added
        sq = src.double().pow(2)
        n = torch.empty_like(sq)
        step = TILE_ROWS if per_input else TILE_COLS
        for a in range(0, sq.shape[dim], step):
            sl = (slice(a, a + step), slice(None)) if per_input else (slice(None), slice(a, a + step))
            n[sl] = sq[sl].sum(dim=dim, keepdim=True).sqrt().expand_as(sq[sl])
    elif defect == "fp32_accumulation":   # a sequential fp32 sum of the squares
        sq, acc = src * src, torch.zeros(in_f if per_input else out_f, dtype=torch.float32)
        for j in range(sq.shape[dim]):
            acc = acc + sq.select(dim, j)
        n = acc.unsqueeze(dim).sqrt().double()
    else:
        n = src.double().pow(2).sum(dim=dim, keepdim=True).sqrt()
    g = d.g.detach().float().double().reshape(-1)
    if defect == "g_by_packed_row":
        assert not per_input
        g = g[packed_row(d.name, torch.arange(out_f)) % out_f]
    g = g[None, :] if per_input else g[:, None]
    m = 1.0 if defect == "drop_m" else float(torch.tensor(d.scale, dtype=torch.float32))
    eps = 0.0 if defect == "drop_eps" else float(torch.tensor(d.eps, dtype=torch.float32))
    den = n + eps
    f = torch.where(den == 0, torch.ones_like(den), 1 + m * (g / den.clamp_min(1e-300) - 1)).float()
    return (v * f).to(torch.bfloat16)
