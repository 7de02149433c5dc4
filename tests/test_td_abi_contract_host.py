"""CPU: the argument contract of the TD entry points (include/nlml_hpe.h, "TD argument checks"), driven through ctypes.

Every check returns before any HIP call, so none of this needs a GPU -- and no case here gets past the checks with N > 0: each
one either fails a check or has N == 0 (no launch, no buffer read).  A host may match on which of two errors it gets, so the ORDER
of the checks is part of the contract: rank -> order -> negative N -> null buffer -> ldx -> fast-order alignment.  The message's
condition wording and the return code are pinned; of its prefix only the operation it names."""
import ctypes as C

import numpy as np
import pytest

from nlml_hpe_amd import _lib

E_BADARG, E_SHAPE = -1, -3
REF, FAST = _lib.TD_ORDER_REFERENCE, _lib.TD_ORDER_FAST
RANK, ORDER, N_NEG, NULL, LDX, ALIGN = "outside [1, 16]", "unknown order", "negative N", "null buffer", "ldx < 1404", "16-byte aligned and ldx % 4 == 0"

# real memory behind every address handed over (nothing may read it, but nothing could fault on it either)
_mem = np.zeros(256, np.uint8)
A16 = (_mem.ctypes.data + 15) & ~15
A4 = A16 + 4

# name -> (operation, takes a rank, takes an order, the buffers that must not be NULL when N > 0)
ENTRY = {
    "nlml_tucker_objective": ("objective", False, False, ("Wm", "x", "params", "cos", "out")),
    "nlml_tucker_objective_ex": ("objective", False, True, ("Wm", "x", "params", "cos", "out")),
    "nlml_tucker_objective_r": ("objective", True, True, ("Wm", "x", "params", "cos", "out")),
    "nlml_tucker_powell": ("powell", False, False, ("Wm", "x", "cos", "out")),
    "nlml_tucker_powell_ex": ("powell", False, True, ("Wm", "x", "cos", "out")),
    "nlml_tucker_powell_r": ("powell", True, True, ("Wm", "x", "cos", "out")),
    "nlml_tucker_gradient_r": ("gradient", True, False, ("Wm", "x", "params", "cos", "out")),
    "nlml_tucker_gradient_host": ("gradient", True, False, ("Wm", "x", "params", "cos", "out")),
}
# (entry point, rank): the rank-aware ones at both ends of the range and at the shipped artefacts' rank
CASES = [(name, r) for name, (_, has_rank, _, _) in ENTRY.items() for r in ((1, 5, 16) if has_rank else (None,))]
WITH_ORDER = [(name, r) for name, r in CASES if ENTRY[name][2]]


def call(name, rank=None, order=REF, N=1, ldx=1404, null=(), **addr):
    """One call with every buffer at a 16-byte aligned address unless `addr` moves it or `null` takes it away -> (rc, message).
    `out` is the one required output: err (objective), result (Powell), grad (gradient); every optional pointer is NULL."""
    op, has_rank, has_order, _ = ENTRY[name]
    p = {k: None if k in null else addr.get(k, A16) for k in ("Wm", "x", "params", "cos", "out")}
    if op == "objective":
        args = [p["Wm"], p["x"], ldx, None, p["params"], p["cos"], N, p["out"], None]
    elif op == "powell":
        args = [p["Wm"], p["x"], ldx, p["cos"], N, None, p["out"], None, None, None, None]
    else:
        args = [p["Wm"], p["x"], ldx, None, p["params"], p["cos"], N, None, p["out"]]
    if has_rank:
        args.append(rank)
    if has_order:
        args.append(order)
    if name == "nlml_tucker_gradient_r":
        args += [None, 0]                     # workspace, workspace_bytes: looked at after the checks pinned here
    args.append(None)                         # stream (nlml_tucker_gradient_host: the optional h_v)
    L = _lib.lib()
    rc = getattr(L, name)(*args)
    return rc, L.nlml_last_error().decode()


def refused(name, code, condition, **kw):
    rc, msg = call(name, **kw)
    assert rc == code, (name, kw, rc, msg)
    assert condition in msg, (name, kw, msg)
    assert msg.startswith("tucker_" + ENTRY[name][0]), (name, msg)   # the operation; the rest of the prefix is the family's


@pytest.mark.parametrize("name", [n for n, e in ENTRY.items() if e[1]])
def test_rank_outside_the_range_is_a_shape_error(name):
    for r in (0, 17, -1):
        for N in (0, 1):
            refused(name, E_SHAPE, RANK, rank=r, N=N)
            assert str(r) in _lib.lib().nlml_last_error().decode()


@pytest.mark.parametrize("name,rank", WITH_ORDER)
def test_unknown_order(name, rank):
    for N in (0, 1):
        refused(name, E_BADARG, ORDER, rank=rank, order=7, N=N)


@pytest.mark.parametrize("name,rank", CASES)
def test_negative_n(name, rank):
    for order in (REF, FAST):
        refused(name, E_BADARG, N_NEG, rank=rank, order=order, N=-1)


@pytest.mark.parametrize("name,rank", CASES)
def test_each_required_buffer(name, rank):
    for buf in ENTRY[name][3]:
        refused(name, E_BADARG, NULL, rank=rank, null=(buf,))
    refused(name, E_BADARG, NULL, rank=rank, null=ENTRY[name][3])


@pytest.mark.parametrize("name,rank", CASES)
def test_short_ldx(name, rank):
    for order in (REF, FAST):
        refused(name, E_BADARG, LDX, rank=rank, order=order, ldx=1403)
    refused(name, E_BADARG, LDX, rank=rank, ldx=0)


@pytest.mark.parametrize("name,rank", WITH_ORDER)
def test_fast_order_alignment(name, rank):
    """Only in the fast order (the reference order reads dwords and takes any 4-byte aligned base and any ldx >= 1404)."""
    refused(name, E_BADARG, ALIGN, rank=rank, order=FAST, Wm=A4)
    refused(name, E_BADARG, ALIGN, rank=rank, order=FAST, x=A4)
    refused(name, E_BADARG, ALIGN, rank=rank, order=FAST, ldx=1405)
    refused(name, E_BADARG, ALIGN, rank=rank, order=FAST, ldx=1406)


@pytest.mark.parametrize("name,rank", CASES)
def test_n_zero_needs_nothing(name, rank):
    """N == 0 with rank and order in range: 0, whatever the buffers, ldx and alignment are -- there is no launch."""
    everything = ("Wm", "x", "params", "cos", "out")
    for order in (REF, FAST):
        assert call(name, rank=rank, order=order, N=0, null=everything)[0] == 0
        assert call(name, rank=rank, order=order, N=0, ldx=3, Wm=A4, x=A4)[0] == 0
        assert call(name, rank=rank, order=order, N=0)[0] == 0


@pytest.mark.parametrize("name,rank", CASES)
def test_the_earlier_check_wins(name, rank):
    """Two conditions at once, for each adjacent pair of the list: the message is the earlier one's."""
    _, has_rank, has_order, need = ENTRY[name]
    if has_rank and has_order:
        refused(name, E_SHAPE, RANK, rank=17, order=7)
    if has_order:
        refused(name, E_BADARG, ORDER, rank=rank, order=7, N=-1)
    for order in (REF, FAST):
        refused(name, E_BADARG, NULL, rank=rank, order=order, null=need[:1], ldx=1403)
    if has_order:
        refused(name, E_BADARG, LDX, rank=rank, order=FAST, ldx=1403, x=A4)
