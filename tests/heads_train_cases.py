"""Shared pieces of the K10 tests (tests/test_heads_train_host.py, tests/test_heads_train_gpu.py): the cases, a Python statement of
the workspace layout, one training step checked launch by launch against the C oracle's model of K9's GEMM order
(oracle/c_oracle.py: et_gemm, et_bias_grad, et_act_grad -- untouched, and sharing no code with csrc/heads_train_ref.h), a numpy model
of the loss, the norm and Adam written from the prose of csrc/heads_train_ref.h, and the reference's loop in torch.

THE PIN.  The caller owns the workspace, and after a call it holds, per network, the last step's resolved rows, A_1..A_5,
delta_1..delta_5 and the f64 norm partials.  So each launch is modelled from the OBSERVED inputs to it and compared word for word
(uint32 / uint64 views: -0 is not +0).  With max_norm = 1e30 the clip coefficient is exactly 1 and the stored gradient is the
gradient the wgrad launches wrote.
"""
import ctypes as C
import functools
import os

import numpy as np
import torch

from nlml_hpe_amd import MLPHeadsTrainer as MT
from nlml_hpe_amd import _lib, synth
from oracle import c_oracle as CO

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (128, 256, 128, 64, 1)
KEYS = [f"model.{2 * i}.{k}" for i in range(5) for k in ("weight", "bias")]
NAMES = ("yaw", "pitch", "roll")
BATCH_MAX = 256
NT = 512
U = 2.0 ** -24
MARGIN = 4.0
FLOOR = 4.0 * U
FILL = np.uint32(0x7FC00000)
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8
NO_CLIP = 1e30
_STREAM_CURVES, _STREAM_STATE = 50, 51
f32 = np.float32


# ---- the layout, stated from the comments of heads_train_ref.h (HtDims, HtWorkspace) ---------------------------------------------------
def dims(R):
    d = {"in": [], "out": list(WIDTHS), "w_off": [], "b_off": [], "part_off": []}
    off, parts, fan_in = 0, 0, R
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


def layout(R, batch):
    """Byte offsets inside ONE network's block: the f64 norm partials (an even number of slots), 256 i32 resolved rows, then A_1..A_5
    and delta_1..delta_5 as dense f32 [batch, out_l], each rounded up to 16 bytes.  Network i's block starts at i * net_bytes."""
    d = dims(R)
    lay = {"partials": 0, "n_partials": d["n_partials"], "act": [], "delta": []}
    off = (d["n_partials"] + 1) // 2 * 2 * 8
    lay["rows"] = off
    off += BATCH_MAX * 4
    for name in ("act", "delta"):
        for w in WIDTHS:
            lay[name].append(off)
            off = -(-(off + batch * w * 4) // 16) * 16
    lay["net_bytes"] = off
    return lay


def workspace_views(ws_bytes, R, batch, net, B):
    lay = layout(R, batch)
    blk = ws_bytes[net * lay["net_bytes"]:(net + 1) * lay["net_bytes"]]
    out = {"partials": blk[:lay["n_partials"] * 8].view(np.float64), "rows": blk[lay["rows"]:lay["rows"] + 4 * B].view(np.int32)}
    for name in ("act", "delta"):
        out[name] = [blk[o:o + batch * w * 4].view(f32).reshape(batch, w)[:B] for o, w in zip(lay[name], WIDTHS)]
    return out


def padding_words(ws_bytes, R, batch, Bs, train=True):
    """-> the words of the workspace that no step may have written: outside the partials, rows[:B] and the [B, out] corners.  Bs: the
    LARGEST batch each network has run (0: the network's whole block)."""
    lay = layout(R, batch)
    words = ws_bytes.view(np.uint32)
    real = np.zeros(words.shape, bool)
    for net, B in enumerate(Bs):
        base = net * lay["net_bytes"] // 4
        if B == 0:
            continue
        if train:
            real[base:base + 2 * lay["n_partials"]] = True
        real[base + lay["rows"] // 4:base + lay["rows"] // 4 + B] = True
        for name in ("act", "delta") if train else ("act",):
            for o, w in zip(lay[name], WIDTHS):
                real[base + o // 4:base + o // 4 + B * w] = True
    return words[~real]


# ---- the data ---------------------------------------------------------------------------------------------------------------------------
def curves(R, seed=0):
    """Cosine parameters f64[R,4] per network: the shipped fits' rows first, further rows drawn around them."""
    td = np.load(os.path.join(REPO, "outputs", "features", "Trained_data.npz"))
    g = synth.rng(seed, _STREAM_CURVES)
    out = {}
    for name in NAMES:
        p = np.asarray(td[f"optimized_{name}"], np.float64)
        extra = p[np.arange(max(0, R - p.shape[0])) % p.shape[0]] * (1.0 + 0.3 * g.standard_normal((max(0, R - p.shape[0]), 4)))
        out[name] = np.concatenate([p, extra])[:R]
    return out


@functools.lru_cache(maxsize=None)
def table(R, rows=(1001, 801, 601), seed=0):
    """{name: (x f32[n,R], y f32[n])}: rows of a cos(b w + c) + d over an even grid of the network's range, as the trainer's table."""
    out = {}
    for name, n, span in zip(NAMES, rows, (50.0, 40.0, 30.0)):
        w = np.radians(np.linspace(-span, span, n).astype(f32))
        p = curves(R, seed)[name]
        x = (p[:, 0] * np.cos(p[:, 1] * w.astype(np.float64)[:, None] + p[:, 2]) + p[:, 3]).astype(f32)
        out[name] = (np.ascontiguousarray(x), np.ascontiguousarray(w, dtype=f32))
    return out


def initial_params(R, seed=0):
    """Kaiming-uniform weights, zero biases -> [flat f32 per network]."""
    sds = MT.initial_state_dicts([R] * 3, seed)
    return [MT.flatten_state_dict(sds[n]) for n in NAMES]


def views(buf, R):
    return MT.state_dict_views(buf, R)


def new_net(x, y, params, order=None, n=None, step0=0, state=None, seed=0):
    """A network of a call as numpy arrays.  state: None (zero grads, m, v) or "warm": m, v of a run in progress (v >= 0)."""
    p = np.array(params, f32)
    net = {"x": x, "y": np.ascontiguousarray(y, f32), "params": p, "grads": np.zeros_like(p), "m": np.zeros_like(p), "v": np.zeros_like(p),
           "order": None if order is None else np.ascontiguousarray(order, np.int32), "step0": int(step0)}
    net["n"] = int(n if n is not None else (len(net["order"]) if order is not None else x.shape[0]))
    if state == "warm":
        g = synth.rng(seed, _STREAM_STATE)
        net["m"] = (1e-3 * g.standard_normal(p.shape)).astype(f32)
        net["v"] = ((1e-3 * g.standard_normal(p.shape)) ** 2).astype(f32)
    return net


def copy_net(net):
    return {k: (v.copy() if isinstance(v, np.ndarray) and k not in ("x", "y") else v) for k, v in net.items()}


def steps_of(n, batch):
    return (n + batch - 1) // batch


# ---- the library's host form through ctypes ------------------------------------------------------------------------------------------
def _ptr(a):
    return a.ctypes.data if a is not None else None


def c_nets(nets, batch, train=True):
    arr = (_lib.HeadsNet * max(1, len(nets)))()
    for i, net in enumerate(nets):
        x = net["x"]
        assert x.dtype == f32 and x.strides[1] == 4 and x.strides[0] % 4 == 0
        steps = steps_of(max(net["n"], 0), batch)
        net["loss"], net["norm"], net["status"] = np.full(steps, np.nan, f32), np.full(steps, np.nan, f32), np.full(1, -1, np.int32)
        a = arr[i]
        a.x, a.ldx, a.N, a.y = _ptr(x), x.strides[0] // 4, x.shape[0], _ptr(net["y"])
        a.params = _ptr(net["params"])
        if train:
            a.grads, a.m, a.v = _ptr(net["grads"]), _ptr(net["m"]), _ptr(net["v"])
        a.order, a.n, a.step0 = _ptr(net["order"]), net["n"], net["step0"]
        a.loss_out, a.norm_out, a.status = _ptr(net["loss"]), _ptr(net["norm"]) if train else None, _ptr(net["status"])
    return arr


def host_train(nets, R, batch, lr=5e-3, weight_decay=1e-5, max_norm=1.0, workspace=True):
    """nlml_heads_train_steps_host on the nets (updated in place; loss, norm, status added) -> the NaN-filled workspace it wrote."""
    ws = np.full(_lib.lib().nlml_heads_train_workspace_bytes(R, batch, len(nets)) // 4, FILL, np.uint32).view(np.uint8) if workspace else None
    arr = c_nets(nets, batch)
    _lib.check(_lib.lib().nlml_heads_train_steps_host(arr, len(nets), R, batch, lr, weight_decay, max_norm, _ptr(ws), ws.size if workspace else 0),
               "nlml_heads_train_steps_host")
    return ws


def host_eval(nets, R, batch, workspace=True):
    ws = np.full(_lib.lib().nlml_heads_train_workspace_bytes(R, batch, len(nets)) // 4, FILL, np.uint32).view(np.uint8) if workspace else None
    arr = c_nets(nets, batch, train=False)
    _lib.check(_lib.lib().nlml_heads_eval_losses_host(arr, len(nets), R, batch, _ptr(ws), ws.size if workspace else 0),
               "nlml_heads_eval_losses_host")
    return ws


# ---- the device form --------------------------------------------------------------------------------------------------------------------
def device_nets(nets, dev, train=True):
    out = []
    for net in nets:
        x = net["x"]
        xd = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        if x.strides[0] // 4 != x.shape[1]:   # keep a padded row stride: the same columns of a wider device tensor
            wide = torch.full((x.shape[0], x.strides[0] // 4), float("nan"), dtype=torch.float32, device=dev)
            wide[:, :x.shape[1]] = xd
            xd = wide[:, :x.shape[1]]
        d = {"x": xd, "y": torch.from_numpy(net["y"]).to(dev), "params": torch.from_numpy(net["params"]).to(dev),
             "order": None if net["order"] is None else torch.from_numpy(net["order"]).to(dev), "n": net["n"], "step0": net["step0"]}
        if train:
            d.update({k: torch.from_numpy(net[k]).to(dev) for k in ("grads", "m", "v")})
        out.append(d)
    return out


def device_train(nets, R, batch, dev, lr=5e-3, weight_decay=1e-5, max_norm=1.0, dnets=None, ws=None):
    """ops.heads_train_steps on copies of the nets (numpy results written back into them) -> (the workspace's bytes, dnets, ws)."""
    from nlml_hpe_amd import ops
    dnets = device_nets(nets, dev) if dnets is None else dnets
    if ws is None:
        ws = torch.full((_lib.lib().nlml_heads_train_workspace_bytes(R, batch, len(nets)) // 4,), float("nan"), dtype=torch.float32, device=dev)
    loss, norm, status = ops.heads_train_steps(dnets, batch=batch, lr=lr, weight_decay=weight_decay, max_norm=max_norm, workspace=ws)
    st = status.cpu().numpy()
    for i, (net, d) in enumerate(zip(nets, dnets)):
        for k in ("params", "grads", "m", "v"):
            net[k] = d[k].cpu().numpy()
        net["loss"], net["norm"], net["status"] = loss[i].cpu().numpy(), norm[i].cpu().numpy(), st[i:i + 1]
    return ws.cpu().numpy().view(np.uint8), dnets, ws


def device_eval(nets, R, batch, dev):
    from nlml_hpe_amd import ops
    ws = torch.full((_lib.lib().nlml_heads_train_workspace_bytes(R, batch, len(nets)) // 4,), float("nan"), dtype=torch.float32, device=dev)
    loss, status = ops.heads_eval_losses(device_nets(nets, dev, train=False), batch=batch, workspace=ws)
    st = status.cpu().numpy()
    for i, net in enumerate(nets):
        net["loss"], net["status"] = loss[i].cpu().numpy(), st[i:i + 1]
    return ws.cpu().numpy().view(np.uint8)


def words(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def same_words(a, b):
    return a.shape == b.shape and np.array_equal(words(a), words(b))


def assert_nets_equal(got, want, what, keys=("params", "grads", "m", "v", "loss", "norm", "status")):
    for i, (g, w) in enumerate(zip(got, want)):
        for k in keys:
            assert same_words(g[k], w[k]), f"{what}: network {i}: {k} differs in {int((words(g[k]) != words(w[k])).sum())} of {g[k].size} words"


# ---- one step, launch by launch, on the C oracle's GEMM order -------------------------------------------------------------------------
def resolve_rows(order, slot0, B, N):
    v = np.arange(slot0, slot0 + B, dtype=np.int64) if order is None else np.asarray(order, np.int64)[slot0:slot0 + B]
    c = np.clip(v, 0, N - 1)
    return c.astype(np.int32), bool((c != v).any())


def relu(z):
    return np.where(z > 0, z, f32(0)).astype(f32)


def check_launches(obs, x, y, params0, grads, R, B, slot0=0, order=None, what=""):
    """obs: workspace_views of a network after ONE step at c = 1; params0: its parameters BEFORE the step; grads: the stored gradient.
    Every forward, wgrad, dgrad and bias gradient from the observed inputs of its launch, word for word -> the count of checks."""
    d = dims(R)
    P = views(params0, R)
    G = views(grads, R)
    rows, _ = resolve_rows(order, slot0, B, x.shape[0])
    assert np.array_equal(obs["rows"], rows), f"{what}: resolved rows"
    n = 0
    for l in range(5):
        W, b = P[f"model.{2 * l}.weight"], P[f"model.{2 * l}.bias"]
        K = d["in"][l]
        if l == 0:
            z = CO.et_gemm(x, W, K, start=b, a_kc=True, b_kc=True, a_rows=rows, M=B)
        else:
            z = CO.et_gemm(obs["act"][l - 1], W, K, start=b, a_kc=True, b_kc=True)
        want = relu(z) if l < 4 else z
        assert same_words(obs["act"][l], want), f"{what}: A_{l + 1} (forward of layer {l}, K = {K}, Nout = {W.shape[0]})"
        n += 1
    for l in range(4, -1, -1):
        dl = obs["delta"][l]
        if l == 0:
            dW = CO.et_gemm(dl, x, B, a_kc=False, b_kc=False, b_rows=rows, N=R)
        else:
            dW = CO.et_gemm(dl, obs["act"][l - 1], B, a_kc=False, b_kc=False)
        assert same_words(G[f"model.{2 * l}.weight"], dW), f"{what}: dW_{l} (wgrad, K = {B}, {dW.shape})"
        assert same_words(G[f"model.{2 * l}.bias"], CO.et_bias_grad(dl)), f"{what}: db_{l}"
        n += 2
        if l:
            s = CO.et_gemm(dl, P[f"model.{2 * l}.weight"], d["out"][l], a_kc=True, b_kc=False)
            assert same_words(obs["delta"][l - 1], CO.et_act_grad(s, obs["act"][l - 1], False)), f"{what}: delta_{l} (dgrad, K = {d['out'][l]})"
            n += 1
    return n


# ---- the loss, the norm and Adam in numpy, written from the prose of heads_train_ref.h -----------------------------------------------
def tree(slots):
    s = slots.copy()
    stride = s.shape[0] // 2
    while stride >= 1:
        s[:stride] = s[:stride] + s[stride:2 * stride]
        stride //= 2
    return s


def model_loss(pred, y, variant=None):
    """pred, y f32[B] -> dict(q [B], slots [256] after the tree, loss, delta5 [B]).  variant "sequential": the q summed b ascending."""
    B = pred.shape[0]
    d = (pred.astype(f32) - y.astype(f32)).astype(f32)
    q = (d * d).astype(f32)
    slots = np.zeros(BATCH_MAX, f32)
    slots[:B] = q
    slots = tree(slots)
    total = slots[0]
    if variant == "sequential":
        total = f32(0)
        for v in q:
            total = f32(total + v)
    return {"q": q, "slots": slots, "loss": f32(total) / f32(B), "delta5": (d * f32(2.0 / B)).astype(f32)}


def model_partials(G, R):
    """The stored (unclipped) gradient as views -> the f64 partial of every wgrad tile, layer 0's tiles first, row-major."""
    out = []
    for l in range(5):
        gW, gb = G[f"model.{2 * l}.weight"].astype(np.float64), G[f"model.{2 * l}.bias"].astype(np.float64)
        for tm in range(-(-gW.shape[0] // 32)):
            for tn in range(-(-gW.shape[1] // 32)):
                tile = np.zeros((32, 32))
                blk = gW[tm * 32:tm * 32 + 32, tn * 32:tn * 32 + 32]
                tile[:blk.shape[0], :blk.shape[1]] = blk
                e = tile.ravel()
                s = np.zeros(NT) + e[:NT] * e[:NT]
                s = s + e[NT:] * e[NT:]
                if tn == 0:
                    b = np.zeros(32)
                    seg = gb[tm * 32:tm * 32 + 32]
                    b[:seg.shape[0]] = seg
                    s[:32] = s[:32] + b * b
                out.append(tree(s)[0])
    return np.array(out)


def model_norm(partials, max_norm):
    chains = np.zeros(NT)
    for i in range(0, partials.shape[0], NT):
        seg = partials[i:i + NT]
        chains[:seg.shape[0]] = chains[:seg.shape[0]] + seg
    norm = np.sqrt(tree(chains)[0])
    c = max_norm / (norm + 1e-6)
    return norm, (c if c < 1.0 else 1.0)


def adam_scales(lr, t):
    return f32(lr / (1.0 - BETA1 ** t)), f32(np.sqrt(1.0 - BETA2 ** t))


def model_adam(p, g, m, v, c, lr, wd, t, variant=None):
    """Every operation a separately rounded float32 one -> (p', g1, m', v').  variants: the deliberately wrong orders."""
    p, g, m, v = (np.asarray(a, f32) for a in (p, g, m, v))
    w1, b2, w2, wdf, eps = f32(1.0 - BETA1), f32(BETA2), f32(1.0 - BETA2), f32(wd), f32(EPS)
    ss, s2 = adam_scales(lr, t)
    g1 = f32(c) * g
    g2 = g1 if variant == "adamw" else g1 + wdf * p
    mn = f32(BETA1) * m + w1 * g2 if variant == "lerp" else m + w1 * (g2 - m)
    vn = b2 * v + w2 * (g2 * g2)
    den = np.sqrt(vn + eps) / s2 if variant == "eps_inside" else np.sqrt(vn) / s2 + eps
    pn = p - ss * (mn / den)
    if variant == "adamw":
        pn = (p - f32(lr) * wdf * p) - ss * (mn / den)
    for a in (g1, mn, vn, pn):
        assert a.dtype == f32
    return pn, g1, mn, vn


VARIANTS = {"sequential": "the loss summed row after row instead of the halving tree", "lerp": "m' = beta1 m + (1 - beta1) g2",
            "eps_inside": "eps under the square root", "adamw": "decoupled (AdamW) weight decay"}


# ---- the reference's loop in torch -------------------------------------------------------------------------------------------------------
def torch_net(sd, dtype):
    return {k: torch.tensor(np.asarray(sd[k]), dtype=dtype, requires_grad=True) for k in KEYS}


def torch_forward(ps, h, pre=None):
    for i in range(5):
        h = torch.nn.functional.linear(h, ps[f"model.{2 * i}.weight"], ps[f"model.{2 * i}.bias"])
        if i < 4:
            if pre is not None:
                pre.append(h)
            h = torch.relu(h)
    return h.squeeze(1)


def relu_margin(sd, x):
    """Per row of x: min over the four ReLU layers' pre-activations of |z| / (16 sqrt(K + 1) 2^-24 R), R = sqrt(sum (a w)^2 + b^2), in
    float64 -- K9's margin (tests/encoder_train_cases.py)."""
    h = torch.from_numpy(np.asarray(x, np.float64))
    worst = torch.full((h.shape[0],), float("inf"), dtype=torch.float64)
    for i in range(4):
        W = torch.from_numpy(np.asarray(sd[f"model.{2 * i}.weight"], np.float64))
        b = torch.from_numpy(np.asarray(sd[f"model.{2 * i}.bias"], np.float64))
        z = h @ W.T + b
        Rr = torch.sqrt((h * h) @ (W * W).T + b * b)
        worst = torch.minimum(worst, (z.abs() / (16.0 * np.sqrt(W.shape[1] + 1.0) * U * Rr)).min(dim=1).values)
        h = torch.relu(z)
    return worst.numpy()


def torch_step(sd, x, y, dtype, max_norm):
    """One step's gradient path -> dict(loss, norm, grads {key: clipped gradient})."""
    ps = torch_net(sd, dtype)
    pred = torch_forward(ps, torch.tensor(x, dtype=dtype))
    loss = torch.nn.MSELoss()(pred, torch.tensor(y, dtype=dtype))
    loss.backward()
    norm = float(torch.nn.utils.clip_grad_norm_(list(ps.values()), max_norm=max_norm))
    return {"loss": float(loss.detach()), "norm": norm, "grads": {k: v.grad.detach().numpy().copy() for k, v in ps.items()}}


def distance(got, exact):
    got, exact = np.asarray(got, np.float64), np.asarray(exact, np.float64)
    den = np.linalg.norm(exact.ravel())
    return float(np.linalg.norm((got - exact).ravel()) / den) if den > 0 else float(np.linalg.norm(got.ravel()))


def check_claim(got, exact, t32, what):
    """The project's bound for K9: every quantity's distance from float64 is at most MARGIN x torch-f32's, with the floor."""
    rows = [(k, got[k], exact[k], t32[k]) for k in ("loss", "norm")] + [(f"grads[{k}]", got["grads"][k], exact["grads"][k], t32["grads"][k]) for k in KEYS]
    bad, worst = [], 0.0
    for name, g, e, t in rows:
        d_g, d_t = distance(g, e), distance(t, e)
        worst = max(worst, d_g / max(d_t, FLOOR / MARGIN))
        if not d_g <= max(MARGIN * d_t, FLOOR):
            bad.append(f"{name}: {d_g:.3e} vs torch-f32 {d_t:.3e}")
    print(f"{what}: worst ratio to torch-f32's distance {worst:.2f}")
    assert not bad, f"{what}: beyond {MARGIN} x torch-f32's distance from the float64 result: " + "; ".join(bad)
    return worst


def gradient_case(R, B, seed=0, net=0):
    """B rows of network `net`'s table that clear K9's ReLU margin under the Kaiming start -> (x, y, params, rejected, candidates)."""
    sds = MT.initial_state_dicts([R] * 3, seed)
    sd = sds[NAMES[net]]
    x, y = table(R)[NAMES[net]]
    pick = synth.rng(seed, _STREAM_STATE + 1).permutation(x.shape[0])[:min(x.shape[0], B + 64)]
    ok = relu_margin(sd, x[pick]) > 1.0
    assert ok.sum() >= B
    used = pick[ok][:B]
    return np.ascontiguousarray(x[used]), np.ascontiguousarray(y[used]), MT.flatten_state_dict(sd), int((~ok).sum()), int(pick.shape[0])


def torch_loop(sds, sets, orders, dtype, batch, lr0, step_size, epochs):
    """The reference's loop (train_network, :83-126) for each network alone, given the split, the orders and the start -> {name:
    (train_loss [epochs], val_loss [epochs], final state dict)}."""
    out = {}
    for name in NAMES:
        ps = torch_net(sds[name], dtype)
        opt = torch.optim.Adam(list(ps.values()), lr=lr0, weight_decay=1e-5)
        sched = torch.optim.lr_scheduler.StepLR(opt, step_size=step_size, gamma=0.9)
        crit = torch.nn.MSELoss()
        (x, y), (xv, yv) = sets[name]["train"], sets[name]["val"]
        tl, vl = [], []
        for epoch in range(epochs):
            o = orders[name][epoch]
            losses = []
            for s in range(0, len(o), batch):
                idx = o[s:s + batch]
                opt.zero_grad()
                loss = crit(torch_forward(ps, torch.tensor(x[idx], dtype=dtype)), torch.tensor(y[idx], dtype=dtype))
                loss.backward()
                torch.nn.utils.clip_grad_norm_(list(ps.values()), max_norm=1.0)
                opt.step()
                losses.append(float(loss.detach()))
            with torch.no_grad():
                vls = [float(crit(torch_forward(ps, torch.tensor(xv[s:s + batch], dtype=dtype)), torch.tensor(yv[s:s + batch], dtype=dtype)))
                       for s in range(0, len(yv), batch)]
            tl.append(sum(losses) / len(losses))
            vl.append(sum(vls) / len(vls))
            sched.step()
        out[name] = (np.array(tl), np.array(vl), {k: v.detach().numpy().copy() for k, v in ps.items()})
    return out
