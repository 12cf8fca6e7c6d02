"""Stage-by-stage float64 reference of the fused MLP kernels, computed from the kernels' own buffers.

A training forward leaves every layer's input in an activation slab (what the consuming step
actually read: save-on-consume, ``mlp_engine.py``) and the backward leaves every hidden layer's dZ
in ``Workspace.dz``.  That is enough to check each kernel stage on ITS OWN inputs:

* encoding features   ``a cos(s x.B)``, ``a sin(s x.B)``, ``x``             (against positions / views)
* a layer's output    ``relu(W a + b)``; a logits head ``W a + b``           (``a``: the slabs it read)
* dZ of a layer       ``mask * sum_consumers W^T dZ_consumer``               (mask: the layer's own slab > 0)
* weight gradients    ``sum_n dZ[n] (x) a[n]``, bias gradients ``sum_n dZ[n]`` (dZ, a: the slabs)

No ReLU sign is recomputed, so none can flip, and what is left of each stage's error is f32
rounding.  Every element is held to ``|got - ref| <= kappa * 2^-24 * sum|terms|``, ``sum|terms|``
being the float64 sum of the absolute products behind that element (for a feature:
``|a| (s sum_d |x_d B_dk| + 1)``: the rounding of the argument plus that of the polynomial).

Exact invariants: padded channels of every slab and dZ slot are 0, dZ rows past ``n`` are 0,
slab rows past ``n`` are finite (a weight-gradient unit multiplies them by those zero dZ rows).

Teeth: every comparison is repeated against a reference with one deliberate change, which must
then fail -- one weight scaled by 1 + 1e-3 (layer outputs, logits, dZ; 1 + 1e-2 in bf16x3), the encoding's scale
scaled by 1 + 1e-3 (features), one row's contribution removed (weight and bias gradients; one
32-sample block's above 10^5 samples).  The weight and the row are the ones the comparison is
most sensitive to, found from the data, so that the check means "a change this small is seen".

Inference launches (no training buffer) leave nothing but logits: ``check_inference`` holds them to
the bits of the training forward's logits of the same kernel organisation, which the stages above
tie to float64.
"""

import torch

U = 2.0 ** -24
TEETH_BLOCK_ABOVE = 100000     # above this many samples the weight-gradient teeth drop a whole block

# kappa per stage and precision, fixed.  Measured on an MI355X over every case of
# tests/test_layer_reference_gpu.py (the headline launch included) and set to about twice the worst
# ratio |err| / (2^-24 sum|terms|) seen, which is given after each value as [exact f32, bf16x6].
# The matrix instructions accumulate up to 1024 products per element in f32: a hidden layer's
# outputs end up a few ulps off (13.8 and 15.6 of 2^-24 sum|terms| at 4M samples), while the weight
# gradients are summed in short segments plus a deterministic reduction and stay smaller.
# bf16x6 is f32-accurate by design and is held to the exact kernels' kappa.
KAPPA = {
    "f32": dict(features=6.0,        # [2.96, 2.92]
                layers=32.0,         # [13.8, 15.6]
                logits=32.0,         # [12.0, 6.81]
                dz=16.0,             # [6.47, 3.69]
                weights=16.0,        # [4.76, 6.50]
                biases=8.0),         # [2.51, 1.90]
    # bf16x3 keeps about 2^-16 of every product (two bf16 parts per operand): the matrix products
    # (layers, dZ, weight gradients) get their own kappa; the features, the logits heads (vector
    # epilogues) and the bias sums are f32 arithmetic as in the exact kernels.  [measured bf16x3]
    "bf16x3": dict(features=6.0,     # [3.00]
                   layers=512.0,     # [226]
                   logits=32.0,      # [4.88]
                   dz=768.0,         # [377]
                   weights=1024.0,   # [427]
                   biases=8.0),      # [1.78]
}
# the deliberate change of one weight (layer outputs, logits, dZ): 1e-3 of it is more than f32
# rounding can explain; in bf16x3 it is below the mode's own 2^-16 per product, so 1e-2 there
TEETH_SCALE = {"f32": 1e-3, "bf16x3": 1e-2}
STAGES = ("features", "layers", "logits", "dz", "weights", "biases")


def kappa_of(precision: str) -> dict:
    return KAPPA["bf16x3" if precision == "bf16x3" else "f32"]


def teeth_scale_of(precision: str) -> float:
    return TEETH_SCALE["bf16x3" if precision == "bf16x3" else "f32"]


class _Stage:
    """Worst ratio, failures and teeth of one stage."""

    def __init__(self, name, kappa):
        self.name, self.kappa = name, kappa
        self.worst = 0.0
        self.failures = []
        self.teeth = {}                     # key -> worst ratio against the changed reference

    def compare(self, key, got, ref, terms, alt=None):
        """``got`` / ``ref`` / ``terms`` (rows, cols) float64; ``alt`` = (column, perturbed
        reference column) or None."""
        if got.numel() == 0:
            return
        err = (got - ref).abs()
        scale = U * terms
        bound = self.kappa * scale
        ok = err <= bound                                   # (NaN fails)
        ratio = torch.where(err == 0, torch.zeros_like(err), err / scale)
        ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
        self.worst = max(self.worst, float(ratio.max()))
        if not bool(ok.all()):
            bad = (~ok).nonzero()[0].tolist()
            self.failures.append("%s %s: %d elements out of bound, first at %s: got %r want %r "
                                 "(bound %.3g)" % (self.name, key, int((~ok).sum()), bad,
                                                   float(got[bad[0], bad[1]]), float(ref[bad[0], bad[1]]),
                                                   float(bound[bad[0], bad[1]])))
        if alt is not None:
            col, alt_ref = alt
            self.note_teeth(key, got[:, col], alt_ref, scale[:, col])

    def note_teeth(self, key, got, alt_ref, scale):
        err = (got - alt_ref).abs()
        r = float(torch.where(err == 0, torch.zeros_like(err), err / scale).max())
        self.teeth[key] = max(self.teeth.get(key, 0.0), r)


def _natural_input(prog, i, slabs):
    """(rows, ld) natural-column input of layer ``i`` from the decoded slabs (float64)."""
    sp = prog.layers[i]
    parts = []
    if sp.act_in > 0:
        parts.append(slabs[prog.slot_of[prog.producer_of[i]]][:, :sp.act_in_p])
    if sp.enc_id is not None:
        parts.append(slabs[prog.enc_slot[sp.enc_id]][:, :prog.encodings[sp.enc_id].width])
    a_int = torch.cat(parts, dim=1)
    cmap = prog.col_maps[i].to(a_int.device).long()
    keep = cmap >= 0
    a_nat = torch.zeros((a_int.shape[0], sp.ld), dtype=torch.float64, device=a_int.device)
    a_nat[:, cmap[keep]] = a_int[:, keep]
    return a_nat


def _features(enc, x):
    """Natural [a cos F | a sin F | x] features of ``x`` (rows, 3) and their sum|terms| (float64)."""
    cols, terms = [], []
    scale = float(enc.scale)
    if enc.num_freq > 0:
        b = enc.b.double().to(x.device)
        a = enc.a.double().to(x.device)
        arg = scale * (x @ b)
        t_arg = abs(scale) * (x.abs() @ b.abs())
        t = a.abs() * (t_arg + 1.0)
        cols += [a * torch.cos(arg), a * torch.sin(arg)]
        terms += [t, t]
    if enc.include_input:
        cols.append(x)
        terms.append(x.abs())
    return torch.cat(cols, 1), torch.cat(terms, 1)


def _feature_alt(enc, x):
    """(natural column, that column with the encoding's scale * (1 + 1e-3)): the most sensitive
    cos column, or the first raw input."""
    if enc.num_freq == 0:
        return 0, x[:, 0] * (1 + 1e-3)
    b = enc.b.double().to(x.device)
    t_arg = x.abs() @ b.abs()
    k = int(t_arg.max(0).values.argmax())
    arg = float(enc.scale) * (1 + 1e-3) * (x @ b[:, k])
    return k, enc.a.double().to(x.device)[k] * torch.cos(arg)


def _pick(score):
    flat = int(torch.nan_to_num(score, nan=0.0).argmax())
    return divmod(flat, score.shape[1])


def check_layers(*args, **kwargs):
    """Checks one forward / backward pair stage by stage (see ``measure_layers``).  Raises
    AssertionError listing every failure (and, with ``teeth``, every comparison a deliberate change
    of the reference did not make fail); returns the report of ``measure_layers``."""
    report, problems = measure_layers(*args, **kwargs)
    assert not problems, "\n".join(problems)
    return report


def measure_layers(prog, positions, views, saved, dz, d_logits, logits, grads, precision="f32",
                   teeth=True, chunk_blocks=1 << 14):
    """One forward / backward pair against float64, stage by stage (see the module docstring).
    ``saved`` is the forward's training buffer, ``dz`` the workspace the backward wrote
    (``Workspace.dz``), ``logits`` the forward's output, ``grads`` the flat gradient buffer.
    Returns ({stage: (worst |err| / (2^-24 sum|terms|), smallest such ratio against a deliberately
    changed reference)}, [problems])."""
    n = int(positions.shape[0])
    dev = positions.device
    kap = kappa_of(precision)
    scale_w = teeth_scale_of(precision)
    st = {s: _Stage(s, kap[s]) for s in STAGES}
    invariants = []
    blocks = (n + 31) // 32
    acts, _ = prog._split_saved(saved, n)
    layers = prog.layers
    hidden = [i for i, sp in enumerate(layers) if sp.to_logits is None]
    consumers = {j: [c for c, p in enumerate(prog.producer_of) if p == j] for j in hidden}
    enc_inputs = {0: positions, 1: views}
    weights = [sp.weight.detach().double().to(dev) for sp in layers]
    biases = [sp.bias.detach().double().to(dev) for sp in layers]
    # natural count of every slot's channels: what lies beyond (or maps to no column) is padding
    real = {}
    for j in hidden:
        real[prog.slot_of[j]] = torch.arange(int(prog.fwd.slot_channels[prog.slot_of[j]]), device=dev) < layers[j].out
    for e, slot in prog.enc_slot.items():
        enc = prog.encodings[e]
        real[slot] = torch.tensor([enc.natural_index(c) >= 0 for c in range(enc.width)], device=dev)
    group = 32 if n > TEETH_BLOCK_ABOVE else 1
    g_acc = {i: [torch.zeros((sp.out, sp.ld), dtype=torch.float64, device=dev),
                 torch.zeros((sp.out, sp.ld), dtype=torch.float64, device=dev),
                 torch.zeros((sp.out,), dtype=torch.float64, device=dev),
                 torch.zeros((sp.out,), dtype=torch.float64, device=dev)] for i, sp in enumerate(layers)}
    g_teeth = {}                 # layer -> (score, weight contribution, bias contribution)
    picks = {}                   # teeth choices, made on the first chunk
    for b0 in range(0, blocks, chunk_blocks):
        nb = min(chunk_blocks, blocks - b0)
        r0, rows = 32 * b0, min(32 * nb, n - 32 * b0)          # valid rows of this chunk
        first = b0 == 0
        slabs, dzs = {}, {}
        for slot in real:
            full = prog.slot_rows(acts, n, slot, b0, nb).double()
            if not bool((full[:, ~real[slot]] == 0).all()):
                invariants.append("slab slot %d: a padded channel is not 0" % slot)
            if not bool(torch.isfinite(full[rows:]).all()):
                invariants.append("slab slot %d: a row past n is not finite" % slot)
            slabs[slot] = full[:rows]
        for j in hidden:
            slot = prog.slot_of[j]
            full = prog.slot_rows(dz, n, slot, b0, nb).double()
            if not bool((full[:, ~real[slot]] == 0).all()):
                invariants.append("dZ of layer %d: a padded channel is not 0" % j)
            if not bool((full[rows:] == 0).all()):
                invariants.append("dZ of layer %d: a row past n is not 0" % j)
            dzs[j] = full[:rows, :layers[j].out]
        dl = d_logits[r0:r0 + rows].double()

        # 1. encoding features
        for e, slot in prog.enc_slot.items():
            enc = prog.encodings[e]
            x = enc_inputs[e][r0:r0 + rows].double()
            ref, terms = _features(enc, x)
            nat = [enc.natural_index(c) for c in range(enc.width)]
            internal = [c for c in range(enc.width) if nat[c] >= 0]
            got = slabs[slot][:, internal]
            order = [nat[c] for c in internal]
            alt = None
            if teeth:
                col, alt_col = _feature_alt(enc, x)
                alt = (order.index(col), alt_col)
            st["features"].compare("encoding %d" % e, got, ref[:, order], terms[:, order], alt)

        # 2. layer outputs and logits
        inputs = {}
        for i, sp in enumerate(layers):
            a = inputs[i] = _natural_input(prog, i, slabs)
            w, b = weights[i], biases[i]
            z = a @ w.T + b
            terms = a.abs() @ w.abs().T + b.abs()
            if sp.to_logits is None:
                got = slabs[prog.slot_of[i]][:, :sp.out]
                ref = torch.relu(z) if sp.relu else z
                stage = "layers"
            else:
                col, cnt = sp.to_logits
                got = logits[r0:r0 + rows, col:col + cnt].double()
                ref = z
                stage = "logits"
            alt = None
            if teeth:
                if first:
                    live = (ref > 0).double() if (sp.relu and sp.to_logits is None) else torch.ones_like(ref)
                    k = min(rows, 8192)
                    picks[("out", i)] = _pick((live[:k] / terms[:k].clamp_min(1e-300)).T @ a[:k].abs() * w.abs())
                o, k = picks[("out", i)]
                zz = z[:, o] + scale_w * w[o, k] * a[:, k]
                alt = (o, torch.relu(zz) if (sp.relu and sp.to_logits is None) else zz)
            st[stage].compare("layer %d" % i, got, ref, terms, alt)

        # 3. dZ: mask * sum over consumers of W^T dZ_consumer, the mask from the layer's own slab
        for j in hidden:
            cons = consumers[j]
            if not cons:
                continue
            out = layers[j].out
            acc = torch.zeros((rows, out), dtype=torch.float64, device=dev)
            terms = torch.zeros_like(acc)
            ups = []
            for c in cons:
                sp = layers[c]
                up = dzs[c] if sp.to_logits is None else dl[:, sp.to_logits[0]:sp.to_logits[0] + sp.to_logits[1]]
                wc = weights[c][:, :out]
                acc += up @ wc
                terms += up.abs() @ wc.abs()
                ups.append((c, up, wc))
            mask = (slabs[prog.slot_of[j]][:, :out] > 0).double() if layers[j].relu else torch.ones_like(acc)
            alt = None
            if teeth:
                if first:
                    k = min(rows, 8192)
                    best = None
                    for c, up, wc in ups:
                        sc = up[:k].abs().T @ (mask[:k] / terms[:k].clamp_min(1e-300)) * wc.abs()
                        o, kk = _pick(sc)
                        if best is None or float(sc[o, kk]) > best[0]:
                            best = (float(sc[o, kk]), c, o, kk)
                    picks[("dz", j)] = best[1:]
                c, o, kk = picks[("dz", j)]
                up, wc = [(u, w_) for cc, u, w_ in ups if cc == c][0]
                alt = (kk, mask[:, kk] * (acc[:, kk] + scale_w * wc[o, kk] * up[:, o]))
            st["dz"].compare("layer %d" % j, dzs[j], mask * acc, mask * terms, alt)

        # 4. weight / bias gradient sums
        for i, sp in enumerate(layers):
            a = inputs[i]
            d = dzs[i] if sp.to_logits is None else dl[:, sp.to_logits[0]:sp.to_logits[0] + sp.to_logits[1]]
            acc = g_acc[i]
            acc[0] += d.T @ a
            acc[1] += d.abs().T @ a.abs()
            acc[2] += d.sum(0)
            acc[3] += d.abs().sum(0)
            if teeth and rows > 0:
                per_row = d.abs().sum(1) * a.abs().sum(1)
                ng = -(-rows // group)
                padded = torch.zeros((ng * group,), dtype=torch.float64, device=dev)
                padded[:rows] = per_row
                scores = padded.view(ng, group).sum(1)
                g = int(scores.argmax())
                if i not in g_teeth or float(scores[g]) > g_teeth[i][0]:
                    lo, hi = g * group, min(g * group + group, rows)
                    g_teeth[i] = (float(scores[g]), d[lo:hi].T @ a[lo:hi], d[lo:hi].sum(0))

    for i, sp in enumerate(layers):
        g, tg, gb, tb = g_acc[i]
        got_w = grads[prog.grad_w_off[i]:prog.grad_w_off[i] + sp.out * sp.ld].view(sp.out, sp.ld).double()
        got_b = grads[prog.grad_b_off[i]:prog.grad_b_off[i] + sp.out].double()
        st["weights"].compare("layer %d" % i, got_w, g, tg)
        st["biases"].compare("layer %d" % i, got_b[None], gb[None], tb[None])
        if teeth and i in g_teeth:
            _, cw, cb = g_teeth[i]
            st["weights"].note_teeth("layer %d" % i, got_w, g - cw, U * tg)
            st["biases"].note_teeth("layer %d" % i, got_b, gb - cb, U * tb)

    problems = list(dict.fromkeys(invariants))
    for s in st.values():
        problems += s.failures
        if teeth:
            problems += ["%s %s: the deliberately changed reference passed too (no teeth: worst ratio "
                         "%.3g, kappa %g)" % (s.name, k, r, s.kappa) for k, r in s.teeth.items() if not r > s.kappa]
    report = {s: (st[s].worst, min(st[s].teeth.values(), default=float("inf"))) for s in STAGES}
    return report, problems


def _logits_head(prog, saved, n, chunk_blocks=1 << 11):
    """The logits heads in float64 on the slabs a training forward left in ``saved``: (logits (n, 4),
    sum|terms| (n, 4)) -- what every kernel organisation that read those slabs may differ by is the
    order in which it added one head's products."""
    dev = saved.device
    acts, _ = prog._split_saved(saved, n)
    heads = [(i, sp) for i, sp in enumerate(prog.layers) if sp.to_logits is not None]
    need = set()
    for i, sp in heads:
        if sp.act_in > 0:
            need.add(prog.slot_of[prog.producer_of[i]])
        if sp.enc_id is not None:
            need.add(prog.enc_slot[sp.enc_id])
    ref = torch.zeros((n, 4), dtype=torch.float64, device=dev)
    terms = torch.zeros((n, 4), dtype=torch.float64, device=dev)
    blocks = (n + 31) // 32
    for b0 in range(0, blocks, chunk_blocks):
        nb = min(chunk_blocks, blocks - b0)
        r0, rows = 32 * b0, min(32 * nb, n - 32 * b0)
        slabs = {slot: prog.slot_rows(acts, n, slot, b0, nb).double()[:rows] for slot in need}
        for i, sp in heads:
            a = _natural_input(prog, i, slabs)
            w = sp.weight.detach().double().to(dev)
            b = sp.bias.detach().double().to(dev)
            col, cnt = sp.to_logits
            ref[r0:r0 + rows, col:col + cnt] = a @ w.T + b
            terms[r0:r0 + rows, col:col + cnt] = a.abs() @ w.abs().T + b.abs()
    return ref, terms


def measure_inference(prog, x, views, logits_train, precision, saved=None):
    """An inference launch (``saved=None``) of the same samples against the training forward's
    ``logits_train`` of the same kernel organisation.  Returns (inference logits, rows whose bits
    differ (bool, n), worst |inference - training| / (2^-24 sum|terms| of the logits head) over those
    rows -- 0.0 when every bit agrees, NaN when they differ and no ``saved`` was given)."""
    got = prog.forward(x, views, None, precision=precision)
    assert got.shape == logits_train.shape and got.dtype == logits_train.dtype
    differs = (got.view(torch.int32) != logits_train.view(torch.int32)).any(dim=1)
    if not bool(differs.any()):
        return got, differs, 0.0
    if saved is None:
        return got, differs, float("nan")
    n = int(x.shape[0])
    _, terms = _logits_head(prog, saved, n)
    err = (got.double() - logits_train.double()).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / (U * terms))
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    return got, differs, float(ratio[differs].max())


def check_inference(prog, x, views, logits_train, precision, saved=None, reordered_from=None):
    """Holds an inference launch to the BITS of the training forward's logits of the same kernel
    organisation (``measure_inference``).  ``reordered_from`` = first row from which the training
    launch is known, from the code, to add a fused head's products in another order than the
    inference launch does (the exact-f32 team kernels of a launch's tail): those rows -- and only
    those -- are held to ``kappa_logits * 2^-24 * sum|terms|`` of the logits head in float64 on the
    training slabs ``saved`` instead; the hidden layers are the same arithmetic, so anything larger
    is a bug.  Returns (inference logits, worst ratio of the rows that differ)."""
    got, differs, worst = measure_inference(prog, x, views, logits_train, precision, saved)
    n = int(x.shape[0])
    exact_rows = n if reordered_from is None else int(reordered_from)
    bad = differs[:exact_rows].nonzero()
    assert bad.numel() == 0, ("inference logits differ from the training forward's in %d of %d rows, first "
                              "row %d: %r != %r (worst ratio to 2^-24 sum|terms| of the head: %.3g)"
                              % (int(bad.numel()), exact_rows, int(bad[0]), got[int(bad[0])].tolist(),
                                 logits_train[int(bad[0])].tolist(), worst))
    if reordered_from is not None and bool(differs.any()):
        assert saved is not None, "the bound on reordered rows needs the training slabs"
        assert worst <= kappa_of(precision)["logits"], (
            "reordered rows: |inference - training| is %.3g x 2^-24 sum|terms| of the logits head "
            "(kappa %g): the hidden layers differ" % (worst, kappa_of(precision)["logits"]))
    return got, worst
