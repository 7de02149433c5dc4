"""K10 without a GPU: the host form of csrc/heads_train_ref.h (nlml_heads_*_host), which the GPU tests hold the device to word for
word, against (1) a Python statement of the workspace layout, (2) the C oracle's model of K9's GEMM order, untouched, (3) a numpy
model of the loss, the norm and Adam written from the header's prose, (4) torch.optim.Adam in float64, (5) float64 autograd under
K9's 4 x torch-f32 claim, (6) the reference's loop, and (7) the argument checks."""
import numpy as np
import pytest
import torch

import heads_train_cases as HC
from nlml_hpe_amd import MLPHeadsTrainer as MT
from nlml_hpe_amd import _lib, synth, weights

U = HC.U


# ---- 1. layout ----------------------------------------------------------------------------------------------------------------------------
def test_workspace_layout_is_the_stated_one():
    L = _lib.lib()
    for R in range(1, 17):
        assert HC.dims(R)["n_partials"] == 78 and HC.dims(R)["total"] == MT.param_count(R)
        for batch in (1, 31, 32, 33, 256):
            for n_nets in (1, 2, 3):
                assert L.nlml_heads_train_workspace_bytes(R, batch, n_nets) == n_nets * HC.layout(R, batch)["net_bytes"], (R, batch, n_nets)
    assert HC.dims(3)["total"] == 74753
    for bad in ((0, 32, 1), (17, 32, 1), (3, 0, 1), (3, 257, 1), (3, 32, 0), (3, 32, 4)):
        assert L.nlml_heads_train_workspace_bytes(*bad) == 0


# ---- 2. the GEMM order, from the oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 3, 5])
def test_every_gemm_of_a_step_is_the_oracles_order(R):
    """One host-form step at c = 1 per batch size; the three networks take B, B', B'' so that every B of the list runs.  Each forward
    (K = R: one super-chunk, waves 1-7 empty; Nout = 1), wgrad (1 x 64 at layer 4), dgrad (K = 1 at layer 4), bias gradient and ReLU
    gradient from the workspace's own inputs to it, word for word."""
    tab, P = HC.table(R), HC.initial_params(R)
    checks = 0
    for rows in ((1, 15, 16), (17, 33, 129), (255, 256, 1)):
        nets = [HC.new_net(*tab[n], P[i], order=synth.rng(R, 80 + i).permutation(tab[n][0].shape[0])[:B].astype(np.int32))
                for i, (n, B) in enumerate(zip(HC.NAMES, rows))]
        before = [n["params"].copy() for n in nets]
        ws = HC.host_train(nets, R, 256, max_norm=HC.NO_CLIP)
        for i, B in enumerate(rows):
            obs = HC.workspace_views(ws, R, 256, i, B)
            checks += HC.check_launches(obs, nets[i]["x"], nets[i]["y"], before[i], nets[i]["grads"], R, B, order=nets[i]["order"],
                                        what=f"R = {R}, B = {B}")
        assert (HC.padding_words(ws, R, 256, rows) == HC.FILL).all()
    assert checks == 9 * 19


# ---- 3. loss, norm, Adam against the numpy model -----------------------------------------------------------------------------------------
CONDITIONS = [dict(max_norm=1.0, state=None, step0=0, wd=1e-5), dict(max_norm=1e3, state="warm", step0=6, wd=1e-5),
              dict(max_norm=1.0, state="warm", step0=6, wd=0.0), dict(max_norm=1e3, state=None, step0=0, wd=0.0)]


def _model_step(net, before, ws_view, R, lr, cond, variant=None):
    """The numpy model of everything after the GEMMs, from the host form's own A_5 and UNCLIPPED gradient (recovered only at c = 1; at
    c < 1 the model runs on a c = 1 twin's gradient, passed in as before['raw'])."""
    B = ws_view["rows"].shape[0]
    loss = HC.model_loss(ws_view["act"][4][:, 0].copy(), net["y"][ws_view["rows"]], variant=variant)
    partials = HC.model_partials(HC.views(before["raw"], R), R)
    norm, c = HC.model_norm(partials, cond["max_norm"])
    pn, g1, mn, vn = HC.model_adam(before["params"], before["raw"], before["m"], before["v"], c, lr, cond["wd"], cond["step0"] + 1, variant=variant)
    return {"loss": np.array([loss["loss"]], np.float32), "delta5": loss["delta5"], "slots": loss["slots"], "q": loss["q"], "partials": partials,
            "norm": np.array([norm], np.float32), "c": c, "grads": g1, "m": mn, "v": vn, "params": pn, "B": B}


@pytest.mark.parametrize("cond", CONDITIONS, ids=lambda c: f"max_norm{c['max_norm']:g}-t{c['step0'] + 1}-wd{c['wd']:g}")
def test_loss_norm_and_adam_are_the_headers_prose(cond):
    R, B, lr = 3, 255, 5e-3      # 255 rows: a sum long enough that the row-after-row variant cannot agree with the tree by luck
    tab, P = HC.table(R), HC.initial_params(R)
    x, y = tab["yaw"]
    net = HC.new_net(x, y, P[0], order=synth.rng(5, 90).permutation(x.shape[0])[:B].astype(np.int32), state=cond["state"], step0=cond["step0"])
    twin = HC.copy_net(net)
    before = {k: net[k].copy() for k in ("params", "m", "v")}
    ws = HC.host_train([net], R, 256, lr=lr, weight_decay=cond["wd"], max_norm=cond["max_norm"])
    HC.host_train([twin], R, 256, lr=0.0, weight_decay=0.0, max_norm=HC.NO_CLIP)
    before["raw"] = twin["grads"]                  # c = 1: the gradient as the wgrad launches left it
    obs = HC.workspace_views(ws, R, 256, 0, B)
    want = _model_step(net, before, obs, R, lr, cond)
    assert (want["c"] < 1.0) == (cond["max_norm"] == 1.0), f"c = {want['c']}: the condition does not hold on these inputs"
    assert HC.same_words(want["partials"], obs["partials"]) and HC.same_words(want["delta5"], obs["delta"][4][:, 0].copy())
    for k in ("loss", "norm", "grads", "m", "v", "params"):
        assert HC.same_words(want[k], net[k]), f"{k}: {int((HC.words(want[k]) != HC.words(net[k])).sum())} words differ from the numpy model"
    assert HC.same_words(want["slots"][:1] / np.float32(B), net["loss"]) and want["q"].shape == (B,)
    # deliberately wrong orders must each change a word here -- or say why they cannot
    for variant, text in HC.VARIANTS.items():
        wrong = _model_step(net, before, obs, R, lr, cond, variant=variant)
        changed = any(not HC.same_words(wrong[k], want[k]) for k in ("loss", "m", "v", "params"))
        if variant == "adamw" and cond["wd"] == 0.0:
            assert not changed, "without weight decay the two decays are the same arithmetic"
        elif variant == "lerp" and cond["state"] is None:
            assert HC.same_words(wrong["m"], want["m"]), "from m = 0 both forms are w1 g2: beta1 * 0 + w1 g2 and 0 + w1 (g2 - 0)"
        else:
            assert changed, f"variant '{text}' changed no word"
    # (a tree over the next power of two >= B instead of 256 slots cannot change a word: the slots b >= B hold +0 and x + 0 is exact)


# ---- 4. it is Adam ---------------------------------------------------------------------------------------------------------------------
def test_the_update_is_torch_adam_in_float64_within_its_roundings():
    """torch.optim.Adam (float64) gets the host form's own clipped gradient g1 as .grad, so only the update is compared.  With
    u = 2^-24, first order, every bound twice (count of f32 roundings on the path) x u x (the magnitudes entering the sum):
      a    = |g1| + |wd p|                                          what enters g2 = g1 + wd p         (2 roundings: wd p, the sum)
      dg2  = 2 * 2 u a
      dm   = 2 * 4 u (|m| + w1 (a + |m|)) + w1 dg2                  w1, g2 - m, w1 (..), m + ..        (4)
      dv   = 2 * 6 u (b2 v + w2 a^2) + 2 w2 a dg2                   b2, w2, b2 v, g2 g2, w2 (..), sum  (6)
      ds   = min(sqrt(dv), dv / sqrt(v'))                           sqrt is concave: never worse than either
      dden = ds / s2 + 2 * 5 u den                                  sqrt, s2, /, eps, +                (5)
      dp   = 2 * 4 u (|p| + T) + 2 (ss dm / den + T dden / den),    T = ss |m'| / den;  ss, /, ss (..), p - ..   (4)
    The term ss dm / den is what makes a free-running comparison of parameters a test of luck: for |g| <~ 1e-7 it is of the size of
    the update itself."""
    R, B, lr, wd, t = 3, 64, 5e-3, 1e-5, 7
    tab, P = HC.table(R), HC.initial_params(R)
    x, y = tab["pitch"]
    net = HC.new_net(x, y, P[1], n=B, state="warm", step0=t - 1)
    p0, m0, v0 = (net[k].astype(np.float64) for k in ("params", "m", "v"))
    HC.host_train([net], R, 256, lr=lr, weight_decay=wd, max_norm=1.0, workspace=False)
    g1 = net["grads"].astype(np.float64)
    p = torch.tensor(p0.copy(), dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([p], lr=lr, weight_decay=wd)
    opt.state[p] = {"step": torch.tensor(float(t - 1)), "exp_avg": torch.tensor(m0.copy()), "exp_avg_sq": torch.tensor(v0.copy())}
    p.grad = torch.tensor(g1.copy())
    opt.step()
    m64, v64, p64 = opt.state[p]["exp_avg"].numpy(), opt.state[p]["exp_avg_sq"].numpy(), p.detach().numpy()
    w1, b2, w2 = 1 - HC.BETA1, HC.BETA2, 1 - HC.BETA2
    ss, s2 = lr / (1 - HC.BETA1 ** t), np.sqrt(1 - HC.BETA2 ** t)
    a = np.abs(g1) + np.abs(wd * p0)
    dg2 = 4 * U * a
    dm = 8 * U * (np.abs(m0) + w1 * (a + np.abs(m0))) + w1 * dg2
    dv = 12 * U * (b2 * v0 + w2 * a * a) + 2 * w2 * a * dg2
    ds = np.minimum(np.sqrt(dv), dv / np.maximum(np.sqrt(v64), 1e-300))
    den = np.sqrt(v64) / s2 + HC.EPS
    dden = ds / s2 + 10 * U * den
    T = ss * np.abs(m64) / den
    dp = 8 * U * (np.abs(p0) + T) + 2 * (ss * dm / den + T * dden / den)
    for name, got, want, bound in (("m'", net["m"], m64, dm), ("v'", net["v"], v64, dv), ("p'", net["params"], p64, dp)):
        err = np.abs(got.astype(np.float64) - want)
        worst = float((err / np.maximum(bound, 1e-300)).max())
        print(f"{name}: worst error / bound {worst:.3f}")
        assert (err <= bound).all(), f"{name}: {int((err > bound).sum())} elements beyond their rounding bound (worst {worst:.2f} x)"


# ---- 5. the gradient path, K9's claim ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 31, 32, 33, 256])
@pytest.mark.parametrize("max_norm", [1.0, 1e3], ids=["clip", "noclip"])
def test_gradient_path_is_within_four_times_torch_f32(B, max_norm):
    R = 3
    x, y, params, rejected, candidates = HC.gradient_case(R, B)
    assert rejected <= 0.05 * candidates, f"{rejected} of {candidates} candidate rows rejected by the ReLU margin"
    net = [HC.new_net(x, y, params)]
    HC.host_train(net, R, 256, max_norm=max_norm, workspace=False)
    sd = HC.views(params, R)
    exact, t32 = HC.torch_step(sd, x, y, torch.float64, max_norm), HC.torch_step(sd, x, y, torch.float32, max_norm)
    assert (exact["norm"] > max_norm) == (max_norm == 1.0)
    got = {"loss": float(net[0]["loss"][0]), "norm": float(net[0]["norm"][0]), "grads": HC.views(net[0]["grads"], R)}
    HC.check_claim(got, exact, t32, f"host, B = {B}, max_norm {max_norm:g}")


# ---- 6. the loop -------------------------------------------------------------------------------------------------------------------------
def _small_tables():
    # 375 / 300 / 225 rows, of which the 80 % that train are 300 / 240 / 180: 3 / 2 / 2 steps at batch 128
    return dict(HC.table(3, rows=(375, 300, 225)))


def test_train_heads_on_the_host_is_the_references_loop(tmp_path):
    """A plumbing check (epoch orders, t carried across calls, StepLR's value per epoch, exhausted networks, the best epoch), not an
    accuracy claim: every epoch mean within 1e-3 relative of the float64 replica of the reference's loop; torch-f32's own distance is
    printed beside it and must stay inside 1e-3 as well."""
    tables = _small_tables()
    kw = dict(tables=tables, epochs=3, batch_size=128, scheduler_step_size=1, verbose=False, config=None, backend="host")
    best, hist = MT.train_heads(None, out_dir=str(tmp_path / "best"), keep="best", **kw)
    last, hist_l = MT.train_heads(None, out_dir=str(tmp_path / "last"), keep="last", **kw)
    assert hist["lr"] == [5e-3, 5e-3 * 0.9, 5e-3 * 0.9 ** 2]
    split = hist["split"]
    sets = {n: {w: (tables[n][0][idx], tables[n][1][idx]) for w, idx in zip(("train", "val"), split[n])} for n in HC.NAMES}
    n_train = [len(split[n][0]) for n in HC.NAMES]
    assert n_train == [300, 240, 180]
    orders = MT.epoch_orders(n_train, 3, 0)
    sds = MT.initial_state_dicts([3, 3, 3], 0)
    exact = HC.torch_loop(sds, sets, orders, torch.float64, 128, 5e-3, 1, 3)
    t32 = HC.torch_loop(sds, sets, orders, torch.float32, 128, 5e-3, 1, 3)
    for name, steps in zip(HC.NAMES, (3, 2, 2)):
        h = hist[name]
        assert [len(s) for s in h["step_loss"]] == [steps] * 3
        for what, got, e, t in (("train", h["train_loss"], exact[name][0], t32[name][0]), ("val", h["val_loss"], exact[name][1], t32[name][1])):
            d_g, d_t = np.abs(np.array(got) - e) / e, np.abs(t - e) / e
            print(f"{name} {what}: host form {d_g.max():.2e}, torch-f32 {d_t.max():.2e} from the float64 loop")
            assert d_g.max() <= 1e-3 and d_t.max() <= 1e-3
        # keep="best" and keep="last" return what they say
        assert h["best_epoch"] == int(np.argmin(h["val_loss"])) + 1 == h["saved_epoch"] and hist_l[name]["saved_epoch"] == 3
        assert hist_l[name]["val_loss"] == h["val_loss"]
        same = all(HC.same_words(best[name][k], last[name][k]) for k in HC.KEYS)
        assert same == (h["best_epoch"] == 3)
        d_last = max(HC.distance(last[name][k], exact[name][2][k]) for k in HC.KEYS if k.endswith("weight"))
        assert d_last < 1e-2, f"{name}: keep='last' is {d_last:.2e} from the float64 loop's final weights"
    # the written files through the unchanged loaders, packed with a synthetic encoder
    for run, sds_run in (("best", best), ("last", last)):
        heads = weights.load_head_state_dicts(str(tmp_path / run))
        enc = synth.encoder_state_dict(136, 0)
        assert weights.validate_shapes(enc, heads) == 136 and weights.pack_blob(enc, heads).size > 0
        assert all(HC.same_words(heads[n][k].numpy(), sds_run[n][k]) for n in HC.NAMES for k in HC.KEYS)


# ---- 7. argument checks ------------------------------------------------------------------------------------------------------------------
def test_argument_checks_in_their_stated_order():
    L = _lib.lib()
    R, batch = 3, 32
    tab, P = HC.table(R), HC.initial_params(R)

    def call(nets=None, n_nets=None, R_=R, batch_=batch, ws_bytes=None, null=None, train=True, lr=5e-3):
        nets = [HC.new_net(*tab[n], P[i], n=40) for i, n in enumerate(HC.NAMES)] if nets is None else nets
        arr = HC.c_nets(nets, max(1, min(batch_, 256)), train=True)
        if null:
            setattr(arr[null[0]], null[1], None)
        need = L.nlml_heads_train_workspace_bytes(R, batch, 3)
        ws = np.zeros(need, np.uint8)
        n_nets = len(nets) if n_nets is None else n_nets
        ws_bytes = need if ws_bytes is None else ws_bytes
        if train:
            rc = L.nlml_heads_train_steps_host(arr if nets else None, n_nets, R_, batch_, lr, 1e-5, 1.0, ws.ctypes.data, ws_bytes)
        else:
            rc = L.nlml_heads_eval_losses_host(arr if nets else None, n_nets, R_, batch_, ws.ctypes.data, ws_bytes)
        return rc, (L.nlml_last_error() or b"").decode()

    def refused(text, **kw):
        rc, msg = call(**kw)
        assert rc != 0 and text in msg, (rc, msg)

    assert call()[0] == 0
    # each check, and before it nothing later in the order: the call also carries every LATER fault
    neg = [HC.new_net(*tab[n], P[i], n=40, step0=-1) for i, n in enumerate(HC.NAMES)]
    refused("n_nets = 0", n_nets=0, R_=0, batch_=0)
    refused("n_nets = 4", n_nets=4)
    refused("R = 17", R_=17, batch_=0)
    refused("R = 0", R_=0)
    refused("batch = 257", batch_=257, null=(0, "x"))
    refused("batch = 0", batch_=0)
    refused("network 1: null buffer", null=(1, "y"), ws_bytes=8, nets=neg)
    refused("network 2: null buffer", null=(2, "m"))
    zero = [HC.new_net(*tab[n], P[i], n=40) for i, n in enumerate(HC.NAMES)]
    zero[1]["n"] = 0
    refused("network 1: n = 0", nets=zero, ws_bytes=8)
    refused("workspace of 8 bytes", ws_bytes=8, nets=neg)
    refused("step0 = -1", nets=neg)
    refused("must be finite", lr=float("nan"))
    assert call(null=(2, "m"), train=False)[0] == 0, "the evaluation pass needs no m"
    rc, msg = call(train=False, ws_bytes=8)
    assert rc != 0 and "workspace of 8 bytes" in msg
    # the device entry points refuse the same way before any GPU call (no GPU is needed to be refused)
    arr = HC.c_nets([HC.new_net(*tab["yaw"], P[0], n=40)], batch)
    assert L.nlml_heads_train_steps(arr, 1, R, batch, 5e-3, 1e-5, 1.0, None, 0, None) != 0 and b"null buffer" in L.nlml_last_error()
    assert L.nlml_heads_train_steps(arr, 0, R, batch, 5e-3, 1e-5, 1.0, None, 0, None) != 0 and b"n_nets = 0" in L.nlml_last_error()
    assert L.nlml_heads_eval_losses(arr, 1, 0, batch, None, 0, None) != 0 and b"R = 0" in L.nlml_last_error()
