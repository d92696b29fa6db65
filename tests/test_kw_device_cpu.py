"""CPU: the batched Wong-Kolter bounds entry points (gnnb_kw_bounds) exist, refuse what they must without a GPU, and the LP producer
knows the "kw_device" bounds mode."""
import ctypes as C

import numpy as np
import pytest
import torch

from gnn_branching_amd import _lib, lp_producer, nets


@pytest.fixture(scope="module")
def lib():
    _lib.build_library()
    return _lib.load()


def test_null_handle_is_refused(lib):
    assert lib.gnnb_kw_workspace_bytes(None, 4) == 0
    kb = _lib.KwBatch()
    out = (C.c_void_p * 4)()
    assert lib.gnnb_kw_bounds(None, C.byref(kb), 4, out, out, None, None, None, None, 0, None) == -1     # GNNB_E_INVALID
    assert b"null handle" in lib.gnnb_last_error()


def test_kw_kernels_have_profile_classes(lib):
    names = [lib.gnnb_profile_class_name(i).decode() for i in range(lib.gnnb_profile_classes())]
    assert {"k_kw_first", "k_kw_layer", "k_kw_flag"} <= set(names) and len(set(names)) == len(names)


def test_kw_device_is_a_bounds_mode():
    nets.register_arch("toy_kw_cpu", [("conv", 3, 4, 4, 2, 1), ("relu",), ("flatten",), ("linear", 4 * 16 * 16, 8), ("relu",), ("linear", 8, 10)], seed=5)
    layers = nets.load_verified_net("toy_kw_cpu", 2, 6)
    x = torch.from_numpy(np.random.RandomState(1).standard_normal((3, 32, 32)).astype(np.float32))
    lp = lp_producer.LayerGraphLP(layers, x - 0.01, x + 0.01, bounds="kw_device")      # no device work until bounds are asked for
    assert lp.bound_mode == "kw_device" and lp.engine is None
    for mode in ("kw", "interval"):
        assert lp_producer.LayerGraphLP(layers, x - 0.01, x + 0.01, bounds=mode).bound_mode == mode
    with pytest.raises(ValueError):
        lp_producer.LayerGraphLP(layers, x - 0.01, x + 0.01, bounds="kw_gpu")


@pytest.mark.parametrize("mode", ["kw", "kw_device"])
def test_parent_without_split_layer_is_refused(mode):
    """A parent always comes with its split: kw_bounds would intersect with it at every layer, kw_device_bounds used to drop it."""
    layers = nets.load_verified_net("cifar_base_kw", 3, 5)
    x = torch.zeros(3, 32, 32)
    lp = lp_producer.LayerGraphLP(layers, x - 0.01, x + 0.01, bounds=mode)
    mask = [torch.full((int(np.prod(lp.shapes[i + 1])),), -1, dtype=torch.long) for i in lp.pre_relu_indices]
    parent = lp.interval_bounds(mask)
    with pytest.raises(ValueError, match="split_layer"):
        lp.bounds(mask, parent, None)
    with pytest.raises(ValueError, match="split_layer"):
        lp.kw_bounds(mask, parent, None)
    with pytest.raises(ValueError, match="split_layer"):
        lp.kw_device_bounds([(mask, None, None), (mask, parent, None)])
    assert lp.engine is None                         # refused before a device is touched
