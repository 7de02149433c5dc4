"""Shared pieces of the K9 order tests (tests/test_encoder_train_order_host.py, tests/test_encoder_train_order_gpu.py): the cases,
a Python statement of the workspace layout, and one training step written launch by launch on the C oracle's order model
(oracle/csrc/oracle.c, "K9": oracle_et_gemm, _bias_grad, _loss, _norm, _update), which shares no code with csrc/encoder_train_ref.h.

THE PIN.  The caller owns the workspace, and after a call of ONE step it holds that step's resolved rows, A_1..A_6, delta_1..delta_6
and the f64 norm partials.  So each of the fourteen launches is modelled from the DEVICE's own inputs to it (`observed`) and compared
word for word (uint32 / uint64 views: -0 is not +0).  Only layer 4's tanh is not reproduced: the model gives Z_4 from the device's
A_4, and the device's A_5 is held to 5 ulp of float64 tanh(Z_4) rounded to f32 (OpenCL's bound for tanh, the one ocml is written to).
Without `observed` the same function chains its own outputs: the whole step, which the host test holds to the host form's values.

THE ELEMENT-WISE BOUND.  A GEMM element is a sum of K products whose every term passes through fewer than K roundings (a wave's chain
and at most seven adds), so it differs from the exact sum by at most gamma_K S <= (K + 2) 2^-24 S, S = sum |a_k b_k| + |start|
(gamma_K = K u / (1 - K u) and K <= 1404).  `chain_bound` returns the float64 value and that bound per element.
"""
import numpy as np

import encoder_train_cases as EC
from nlml_hpe_amd import _lib
from oracle import c_oracle as CO

WIDTHS = EC.WIDTHS
BATCH_MAX = 256
LATENT, LATENT_LD = 9, 12
FILL = np.uint32(0x7FC00000)       # the word torch.full(.., nan, dtype=float32) writes
U = 2.0 ** -24
TANH_ULP = 5                       # OpenCL's bound for tanh, not the measurement (profiles/encoder_train.md has that)

# (F, B): the smallest shapes at which each edge of the order exists
#   B = 1            wgrad K = 1, fifteen empty bias runs          B = 129       spw = 2, wave 4 holds one row
#   B = 15, 16, 17   the second super-chunk and wave 1 appear      B = 241, 255  the last bias run has 1 and 15 rows
#   B = 33           two tiles of rows                             B = 256       the full batch
#   F = 1404         a 28-column partial tile, spw = 11 (at B = 33 only: the step is 0.3 GFLOP of scalar C)
# F = 136 gives a half super-chunk in layer 0 (k 128..135 on wave 4); layer 5 gives Nout = 9 and a dgrad with K = 9.
SHAPES = [(136, 1), (136, 15), (136, 16), (136, 17), (136, 33), (136, 129), (136, 241), (136, 255), (136, 256), (1404, 33)]
NO_CLIP = dict(lr=0.0, weight_decay=0.0, max_norm=1e30, zero_grad=False)   # c is exactly 1 and the parameters stay
VARIANTS = {1: "natural k order inside a super-chunk", 2: "wave partials added as a halving tree", 3: "spw = floor(nsc / 8)",
            4: "bias added after the wave sum", 5: "bias runs of a fixed 16 rows", 6: "loss tree over B slots",
            7: "tile norm partials in f32", 8: "c g contracted into the update's fmaf"}


# ---- the layout, stated from the comments of encoder_train_ref.h (EtDims, EtWorkspace) ------------------------------------------------
def dims(F):
    """Offsets in floats of W_l [out, in] and b_l [out] in the flat params / grads buffers, and the first norm partial of layer l."""
    d = {"in": [], "out": list(WIDTHS), "w_off": [], "b_off": [], "part_off": []}
    off, parts, fan_in = 0, 0, F
    for w in WIDTHS:
        d["in"].append(fan_in)
        d["w_off"].append(off)
        off += w * fan_in
        d["b_off"].append(off)
        off += w
        d["part_off"].append(parts)
        parts += -(-w // 32) * -(-fan_in // 32)
        fan_in = w
    d["total"], d["n_partials"] = off, parts
    return d


def layout(F, batch):
    """Byte offsets inside the workspace of one batch: the f64 norm partials (an even number of slots), 256 i32 resolved rows, then
    A_1..A_6 and delta_1..delta_6 as f32 [batch, ld] (ld = the layer's width, 12 for the last), each rounded up to 16 bytes."""
    d = dims(F)
    lay = {"partials": 0, "n_partials": d["n_partials"], "ld": [LATENT_LD if w == LATENT else w for w in WIDTHS], "act": [], "delta": []}
    off = (d["n_partials"] + 1) // 2 * 2 * 8
    lay["rows"] = off
    off += BATCH_MAX * 4
    for name in ("act", "delta"):
        for ld in lay["ld"]:
            lay[name].append(off)
            off = -(-(off + batch * ld * 4) // 16) * 16
    lay["bytes"] = off
    return lay


def workspace_views(ws_bytes, F, batch, B):
    """ws_bytes: uint8 array of the read-back workspace -> dict(partials f64, rows i32[B], act / delta: six f32 [B, out] views)."""
    lay, out = layout(F, batch), {}
    out["partials"] = ws_bytes[:lay["n_partials"] * 8].view(np.float64)
    out["rows"] = ws_bytes[lay["rows"]:lay["rows"] + 4 * B].view(np.int32)
    for name in ("act", "delta"):
        out[name] = [ws_bytes[o:o + batch * ld * 4].view(np.float32).reshape(batch, ld)[:B, :w] for o, ld, w in zip(lay[name], lay["ld"], WIDTHS)]
    return out


def padding_report(ws_bytes, F, batch, B):
    """-> (padding words that are no longer FILL, real elements that are not finite).  Real: the n_partials f64 slots, rows[:B], and
    the [B, out] corner of every A_l / delta_l; everything else (the odd partial slot, rows >= B, columns 9..11 of the last layer,
    the bytes that round a tensor up to 16) is padding."""
    lay = layout(F, batch)
    words = ws_bytes[:lay["bytes"]].view(np.uint32)
    real = np.zeros(words.shape, bool)
    real[:2 * lay["n_partials"]] = True
    real[lay["rows"] // 4:lay["rows"] // 4 + B] = True
    nonfinite = int((~np.isfinite(ws_bytes[:lay["n_partials"] * 8].view(np.float64))).sum())
    for name in ("act", "delta"):
        for o, ld, w in zip(lay[name], lay["ld"], WIDTHS):
            m = real[o // 4:o // 4 + batch * ld].reshape(batch, ld)
            m[:B, :w] = True
            nonfinite += int((~np.isfinite(words[o // 4:o // 4 + batch * ld].view(np.float32).reshape(batch, ld)[:B, :w])).sum())
    return int((words[~real] != FILL).sum()), nonfinite


# ---- the data of a step ----------------------------------------------------------------------------------------------------------------
def resolve_rows(order, slot0, B, N):
    """The dataset rows of the batch slots [slot0, slot0 + B): order[slot] (None: the slot) clamped into [0, N) -> (rows i32, clamped)."""
    v = np.arange(slot0, slot0 + B, dtype=np.int64) if order is None else np.asarray(order, np.int64)[slot0:slot0 + B]
    c = np.clip(v, 0, N - 1)
    return c.astype(np.int32), bool((c != v).any())


def targets(cs, rows, labels=None):
    """f32[B, 9]: the three table rows the (clamped) labels of `rows` name, side by side."""
    lab = (cs["labels"] if labels is None else labels)[rows]
    return np.concatenate([t[np.clip(lab[:, i], 0, t.shape[0] - 1)] for i, t in enumerate(cs["tables"])], axis=1).astype(np.float32)


def relu(z):
    return np.where(z > 0, z, np.float32(0)).astype(np.float32)


def model_step(x, rows, target, params, grads, F, hyper, observed=None, variant=0):
    """One step on the order model.  x f32[N, >=F] (rows may be strided), rows i32[B], target f32[B, 9], params / grads the flat f32
    buffers BEFORE the step, hyper: lr, weight_decay, max_norm, zero_grad.
    observed (workspace_views of the device's step): every launch takes its inputs from it, and act[4] (tanh) is not modelled.
    observed None: every launch takes the model's own outputs, with this machine's tanhf for layer 4 (the host form's).
    -> dict(z, act, delta, dsum [six each], q, loss, g_pre, partials, norm (f32), norm64, c, p_out, g_out)."""
    d, B = dims(F), len(rows)
    x = x[:, :F]
    P = [(params[d["w_off"][l]:d["b_off"][l]].reshape(d["out"][l], d["in"][l]), params[d["b_off"][l]:d["b_off"][l] + d["out"][l]]) for l in range(6)]
    m = {"z": [None] * 6, "act": [None] * 6, "delta": [None] * 6, "dsum": [None] * 6}
    a_in = observed["act"] if observed else m["act"]
    d_in = observed["delta"] if observed else m["delta"]
    for l in range(6):
        z = CO.et_gemm(x if l == 0 else a_in[l - 1], P[l][0], d["in"][l], start=P[l][1], a_kc=True, b_kc=True, a_rows=rows if l == 0 else None,
                       M=B, variant=variant)
        m["z"][l] = z
        m["act"][l] = relu(z) if l < 4 else (z if l == 5 else (None if observed else CO.et_tanhf(z)))
    ls = CO.et_loss(a_in[5], target, variant=variant)
    m["q"], m["loss"], m["delta"][5] = ls["q"], ls["loss"], ls["delta6"]
    g_pre = np.array(grads, np.float32, copy=True)
    for l in range(5, -1, -1):
        out, fan_in = d["out"][l], d["in"][l]
        a_prev = x if l == 0 else a_in[l - 1]
        dW = CO.et_gemm(d_in[l], a_prev, B, a_kc=False, b_kc=False, b_rows=rows if l == 0 else None, M=out, N=fan_in, variant=variant)
        db = CO.et_bias_grad(d_in[l], variant=variant)
        for off, val in ((d["w_off"][l], dW.ravel()), (d["b_off"][l], db)):
            g_pre[off:off + val.size] = val if hyper["zero_grad"] else g_pre[off:off + val.size] + val
        if l:
            m["dsum"][l] = CO.et_gemm(d_in[l], P[l][0], out, a_kc=True, b_kc=False, M=B, N=fan_in, variant=variant)
            m["delta"][l - 1] = CO.et_act_grad(m["dsum"][l], a_in[l - 1], l - 1 == 4)
    nm = CO.et_norm(F, G=g_pre, max_norm=hyper["max_norm"], variant=variant)
    m["g_pre"], m["partials"] = g_pre, nm["partials"]
    if observed:   # the update launch reads the device's partials
        nm = CO.et_norm(F, partials=observed["partials"], max_norm=hyper["max_norm"])
    m["norm64"], m["norm"], m["c"] = nm["norm"], np.float32(nm["norm"]), nm["c"]
    m["p_out"], m["g_out"] = CO.et_update(params, g_pre, np.float32(nm["c"]), hyper["lr"], hyper["weight_decay"], variant=variant)
    return m


def words(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def mismatches(a, b):
    """The number of words in which two arrays of one shape and type differ (-0 is not +0)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    return int((words(a) != words(b)).sum())


def ulp_distance(a, b):
    """Per element: how many f32 values lie between a and b (0: the same value)."""
    def key(v):
        i = np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def chain_bound(A, Bm, start=None):
    """float64 A @ Bm (+ start) and the bound (K + 2) 2^-24 (|A| @ |Bm| + |start|), element by element."""
    A, Bm = np.asarray(A, np.float64), np.asarray(Bm, np.float64)
    ref, S = A @ Bm, np.abs(A) @ np.abs(Bm)
    if start is not None:
        ref, S = ref + np.asarray(start, np.float64), S + np.abs(np.asarray(start, np.float64))
    return ref, (A.shape[1] + 2) * U * S


def pin_step(cs, rows, before, after, ws_bytes, batch, loss, norm, hyper, labels=None, x=None, accuracy=True):
    """Hold one device step to the model, launch by launch.  before / after: (params, grads) flat f32 around the step; ws_bytes: the
    workspace after it; loss, norm: the step's f32 outputs.  -> (dict quantity -> mismatching words, dict of measurements).
    accuracy: also hold every observable GEMM element to chain_bound (the wgrad through G, so only where G was zero and c is 1)."""
    F, B = cs["F"], len(rows)
    x = cs["x"] if x is None else x
    obs = workspace_views(ws_bytes, F, batch, B)
    m = model_step(x, rows, targets(cs, rows, labels), before[0], before[1], F, hyper, observed=obs)
    bad = {"rows": mismatches(obs["rows"], np.asarray(rows, np.int32))}
    for l in (0, 1, 2, 3, 5):
        bad[f"A_{l + 1}"] = mismatches(obs["act"][l], m["act"][l])
    ulp = ulp_distance(obs["act"][4], np.tanh(m["z"][4].astype(np.float64)).astype(np.float32))
    info = {"tanh_ulp": int(ulp.max())}
    bad["A_5 beyond 5 ulp"] = int((ulp > TANH_ULP).sum())
    bad["loss"] = mismatches(np.float32(loss), np.float32(m["loss"]))
    for l in range(6):
        bad[f"delta_{l + 1}"] = mismatches(obs["delta"][l], m["delta"][l])
    bad["partials"] = mismatches(obs["partials"], m["partials"])
    bad["norm"] = mismatches(np.float32(norm), m["norm"])
    c32 = np.float32(m["c"])
    info["c"] = float(c32)
    bad["G_out"] = mismatches(after[1], (c32 * m["g_pre"]).astype(np.float32))
    bad["G_out (update model)"] = mismatches(after[1], m["g_out"])
    bad["p_out"] = mismatches(after[0], m["p_out"])
    pad, nonfinite = padding_report(ws_bytes, F, batch, B)
    bad["padding words overwritten"], bad["non-finite real elements"] = pad, nonfinite
    if accuracy:
        d = dims(F)
        xr = x[:, :F][rows]
        beyond = 0
        for l in range(6):
            W = before[0][d["w_off"][l]:d["b_off"][l]].reshape(d["out"][l], d["in"][l])
            bias = before[0][d["b_off"][l]:d["b_off"][l] + d["out"][l]]
            a_prev = xr if l == 0 else obs["act"][l - 1]
            if l != 4:   # forward: through the ReLU, which moves no value further from relu(ref) than it was from ref
                ref, bound = chain_bound(a_prev, W.T, bias)
                beyond += int((np.abs(obs["act"][l] - (np.maximum(ref, 0) if l < 4 else ref)) > bound).sum())
            if l:        # dgrad: times act' (0 / 1, or the tanh layer's fmaf(-a, a, 1) in [0, 1] and one more rounding)
                ref, bound = chain_bound(obs["delta"][l], W)
                f = CO.et_act_grad(np.ones_like(obs["act"][l - 1]), obs["act"][l - 1], l - 1 == 4).astype(np.float64)
                extra = 2 * U * np.abs(ref * f) if l - 1 == 4 else 0.0
                beyond += int((np.abs(obs["delta"][l - 1] - ref * f) > bound * f + extra).sum())
            if c32 == 1 and not before[1].any():
                ref, bound = chain_bound(obs["delta"][l].T, a_prev)
                beyond += int((np.abs(after[1][d["w_off"][l]:d["b_off"][l]].reshape(ref.shape) - ref) > bound).sum())
        bad["GEMM elements beyond the chain bound"] = beyond
    return bad, info


def assert_pinned(bad, what):
    print(f"{what}: mismatching words {sum(bad.values())} of {len(bad)} pinned quantities")
    wrong = {k: v for k, v in bad.items() if v}
    assert not wrong, f"{what}: words that differ from the order model: {wrong}"


# ---- the device ------------------------------------------------------------------------------------------------------------------------
def nan_workspace(F, batch, dev):
    import torch
    need = _lib.lib().nlml_encoder_train_workspace_bytes(F, batch)
    assert need % 4 == 0
    return torch.full((need // 4,), float("nan"), dtype=torch.float32, device=dev)


def ws_bytes_of(ws):
    return ws.cpu().numpy().view(np.uint8)


def device_call(cs, dev, order, batch, p, g, hyper, ws=None, x=None, labels=None, tabs=None):
    """ops.encoder_train_steps on the device buffers p, g (updated in place) -> (loss, norm f32 arrays, status, workspace tensor)."""
    import torch
    from nlml_hpe_amd import ops
    xd = torch.from_numpy(cs["x"]).to(dev) if x is None else x
    lab = torch.from_numpy(cs["labels"] if labels is None else labels).to(dev)
    tabs = [torch.from_numpy(t).to(dev) for t in cs["tables"]] if tabs is None else tabs
    od = None if order is None else torch.from_numpy(np.ascontiguousarray(order, np.int32)).to(dev)
    ws = nan_workspace(cs["F"], batch, dev) if ws is None else ws
    loss, norm, status = ops.encoder_train_steps(xd, lab, tabs, p, g, order=od, batch=batch, workspace=ws, **hyper)
    return loss.cpu().numpy(), norm.cpu().numpy(), int(status.cpu()[0]), ws


def fresh(cs, dev):
    import torch
    p = torch.from_numpy(cs["params"]).to(dev)
    return p, torch.zeros_like(p)


def state(p, g):
    return p.cpu().numpy().copy(), g.cpu().numpy().copy()
