"""engine.check_batch: the one size rule of a scorer batch, on CPU tensors, numpy arrays and ScorerEngine._HostBuf objects, against the
three checks it replaces (restated below as they stood: ScorerEngine._marshal, the body of forward_host, HostFedPipeline._check_sizes)."""
import numpy as np
import pytest
import torch
from torch import nn

from gnn_branching_amd.engine import ScorerEngine, check_batch
from gnn_branching_amd.plnn.modules import Flatten

# cifar_base_kw at B = 2: conv 3->8 and 8->16 (4x4, stride 2, pad 1) on 3x32x32, Linear 1024 -> 100
SIZES, R, B = [3072, 2048, 1024, 100, 1], 3172, 2
FIXED = [nn.Conv2d(3, 8, 4, 2, 1), nn.ReLU(), nn.Conv2d(8, 16, 4, 2, 1), nn.ReLU(), Flatten(), nn.Linear(1024, 100), nn.ReLU()]
PRIMALS = [B * 2048, B * 2048, B * 1024, B * 1024, 7, B * 100, B * 100, B]      # primals[4] (behind Flatten) is read by nobody: any size
GROUPS = ("lbs", "ubs", "duals", "prim")


def valid():
    """The element counts of a valid batch, per group."""
    return {"lbs": [B * n for n in SIZES], "ubs": [B * n for n in SIZES], "duals": [3 * B * n for n in SIZES[1:-1]], "prim": list(PRIMALS),
            "x_lp": B * SIZES[0], "mask": B * R}


def cases():
    """(name, element counts, refused by (new rule, old _marshal, old forward_host, old _check_sizes)) -- verdicts written by hand."""
    every = (True,) * 4
    out = [("valid", valid(), (False,) * 4)]
    other = valid()
    other["prim"][4] = 1
    out.append(("unread primal of another size", other, (False,) * 4))
    for g in GROUPS:
        for k in range(len(valid()[g])):
            if g == "prim" and k == 4:
                continue
            for d in (-1, 1):
                c = valid()
                c[g][k] += d
                out.append((f"{g}[{k}]{d:+d}", c, every))
        few, many = valid(), valid()
        few[g].pop(-2 if g == "prim" else -1)                 # (primals: the last one stays the last)
        # one tensor too many, of the size the old loops would have expected at that index where they had one: 3 B N_4 for a fourth dual
        many[g].append(3 * B * SIZES[-1] if g == "duals" else many[g][-1])
        # the number of dual tensors was checked by _check_sizes alone (through forward a missing one was the C side's RuntimeError)
        verdict = (True, False, False, True) if g == "duals" else every
        out += [(f"one {g} tensor too few", few, verdict), (f"one {g} tensor too many", many, verdict)]
    for name in ("mask", "x_lp"):
        for d in (-1, 1):
            c = valid()
            c[name] += d
            out.append((f"{name}{d:+d}", c, every))
    return out


CASES = cases()


def carriers(c):
    """The batch of element counts c as CPU tensors, as numpy arrays and as _HostBuf objects."""
    def tree(make):
        return {k: [make(n) for n in v] if isinstance(v, list) else make(v) for k, v in c.items()}
    return {"tensor": tree(lambda n: torch.zeros(n)), "numpy": tree(lambda n: np.zeros(n, np.float32)),
            "hostbuf": tree(lambda n: ScorerEngine._HostBuf(torch.zeros(n)))}


# ---- the three old checks, as they stood --------------------------------------------------------------------------------------------------
def old_check_primals(sizes, fixed, prim, B):
    def count(t):
        return t.numel() if torch.is_tensor(t) else t.size      # (tensors, numpy arrays, _HostBuf)
    if len(prim) != len(fixed) + 1:
        raise ValueError(f"{len(prim)} primal tensors for {len(fixed) + 1} network layers")
    k = 0
    for q, l in enumerate(fixed):
        if type(l) is nn.ReLU:
            k += 1
            n = B * sizes[k]
            if count(prim[q - 1]) != n or count(prim[q]) != n:
                raise ValueError(f"primals[{q - 1}], primals[{q}] must hold {n} values each")
    if count(prim[-1]) != B:
        raise ValueError("primals[-1] must hold one value per subproblem")


def old_marshal(sizes, R, fixed, B, lbs, ubs, duals, prim, x_lp, mask):        # device tensors there; CPU tensors here
    ng = len(sizes)
    if len(lbs) != ng or len(ubs) != ng:
        raise ValueError(f"{len(lbs)} bound tensors, layer graph has {ng} layers")
    for k, (l, u) in enumerate(zip(lbs, ubs)):
        if l.numel() != B * sizes[k] or u.numel() != B * sizes[k]:
            raise ValueError(f"bounds of graph layer {k}: {tuple(l.shape)} does not hold {B}x{sizes[k]} values")
    for k, d in enumerate(duals):
        if d.numel() != B * sizes[k + 1] * 3:
            raise ValueError(f"dual_vars[{k}] has {tuple(d.shape)}, expected ({B * sizes[k + 1]}, 3)")
    if mask.numel() != B * R:
        raise ValueError(f"masks has {tuple(mask.shape)}, expected ({B}, {R})")
    if x_lp.numel() != B * sizes[0]:
        raise ValueError("primal_inputs has the wrong size")
    old_check_primals(sizes, fixed, prim, B)


def old_forward_host(sizes, R, fixed, B, lbs, ubs, duals, prim, x_lp, mask):   # _HostBuf objects
    ng = len(sizes)
    if len(lbs) != ng or len(ubs) != ng:
        raise ValueError(f"{len(lbs)} bound tensors, layer graph has {ng} layers")
    for k, (l, u) in enumerate(zip(lbs, ubs)):
        if l.size != B * sizes[k] or u.size != B * sizes[k]:
            raise ValueError(f"bounds of graph layer {k}: {l.size} values, expected {B}x{sizes[k]}")
    for k, d in enumerate(duals):
        if d.size != B * sizes[k + 1] * 3:
            raise ValueError(f"dual_vars[{k}] has {d.size} values, expected ({B * sizes[k + 1]}, 3)")
    if mask.size != B * R:
        raise ValueError(f"masks has {mask.size} values, expected ({B}, {R})")
    if x_lp.size != B * sizes[0]:
        raise ValueError("primal_inputs has the wrong size")
    old_check_primals(sizes, fixed, prim, B)


def old_check_sizes(sizes, R, fixed, B, lbs, ubs, duals, prim, x_lp, mask):    # host tensors, addressed in submit's flat list
    host = list(lbs) + list(ubs) + list(duals) + list(prim) + [x_lp, mask]
    nb, nd, npr = len(lbs), len(duals), len(prim)
    if nb != len(sizes) or nd != len(sizes) - 2:
        raise ValueError(f"{nb} bound tensors / {nd} dual tensors, layer graph has {len(sizes)} layers")
    for k in range(nb):
        for t, what in ((host[k], "lower"), (host[nb + k], "upper")):
            if t.numel() != B * sizes[k]:
                raise ValueError(f"{what} bounds of graph layer {k}: {tuple(t.shape)} does not hold {B}x{sizes[k]} values")
    for k in range(nd):
        if host[2 * nb + k].numel() != B * sizes[k + 1] * 3:
            raise ValueError(f"dual_vars[{k}] has {tuple(host[2 * nb + k].shape)}, expected ({B * sizes[k + 1]}, 3)")
    old_check_primals(sizes, fixed, host[2 * nb + nd:2 * nb + nd + npr], B)
    if host[-1].numel() != B * R:
        raise ValueError(f"masks has {tuple(host[-1].shape)}, expected ({B}, {R})")
    if host[-2].numel() != B * sizes[0]:
        raise ValueError("primal_inputs has the wrong size")


def refuses(check, t):
    try:
        check(SIZES, R, FIXED, B, t["lbs"], t["ubs"], t["duals"], t["prim"], t["x_lp"], t["mask"])
    except ValueError:
        return True
    return False


@pytest.mark.parametrize("name,c,refused", CASES, ids=[c[0].replace(" ", "_") for c in CASES])
def test_check_batch_and_the_checks_it_replaces(name, c, refused):
    """The valid batch passes and every wrong count raises ValueError, in all three carriers; the old checks, each on the carrier it
    saw, give the same verdict -- but for the number of dual tensors, which only _check_sizes looked at."""
    new, marshal, forward_host, check_sizes = refused
    by = carriers(c)
    for kind, t in by.items():
        assert refuses(check_batch, t) == new, kind
    assert refuses(old_marshal, by["tensor"]) == marshal
    assert refuses(old_forward_host, by["hostbuf"]) == forward_host
    assert refuses(old_check_sizes, by["tensor"]) == check_sizes


def test_the_babsr_subset():
    """babsr has bounds and a mask only: the other groups are None and not looked at; its own groups are still checked."""
    short = carriers(dict(valid(), mask=B * R - 1))
    for kind, t in carriers(valid()).items():
        check_batch(SIZES, R, FIXED, B, t["lbs"], t["ubs"], mask=t["mask"])
        with pytest.raises(ValueError, match="masks"):
            check_batch(SIZES, R, FIXED, B, t["lbs"], t["ubs"], mask=short[kind]["mask"])
        with pytest.raises(ValueError, match="upper_bounds_all: 4 tensors, expected 5"):
            check_batch(SIZES, R, FIXED, B, t["lbs"], t["ubs"][:-1], mask=t["mask"])


def test_messages_name_the_argument_and_the_expected_count():
    t = carriers(valid())["numpy"]
    with pytest.raises(ValueError, match=r"dual_vars\[1\] holds 6143 values, expected 6144"):
        check_batch(SIZES, R, FIXED, B, t["lbs"], t["ubs"], t["duals"][:1] + [t["duals"][1][:-1]] + t["duals"][2:], t["prim"], t["x_lp"], t["mask"])
    with pytest.raises(ValueError, match=r"dual_vars: 2 tensors, expected 3"):
        check_batch(SIZES, R, FIXED, B, t["lbs"], t["ubs"], t["duals"][:-1], t["prim"], t["x_lp"], t["mask"])
