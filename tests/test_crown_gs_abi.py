"""CPU checks of the activation-parameterised CROWN entry points (fiode_certify_crown_act,
fiode_certify_crown_workspace_bytes_act) and of the ops.groupsort_crown() switch."""
import ctypes as ct
import pathlib
import re

import pytest
import torch

ROOT = pathlib.Path(__file__).resolve().parents[1]
SYMBOLS = ("fiode_certify_crown_act", "fiode_certify_crown_workspace_bytes_act")
EINVAL, ESHAPE, EWORKSPACE = 1, 2, 3
RELU, GROUPSORT = 0, 1


def test_header_declares_and_library_exports_the_symbols():
    from fiode_amd import _lib
    text = (ROOT / "include" / "fiode.h").read_text()
    declared = re.findall(r"FIODE_API\s+[\w\s\*]+?\b(fiode_\w+)\s*\(", text)
    lib = ct.CDLL(str(_lib.LIB_PATH))
    for s in SYMBOLS:
        assert s in declared and hasattr(lib, s), s
    assert _lib.lib().fiode_abi_version() == _lib.ABI_VERSION == 5           # new symbols only
    assert (_lib.FIODE_ACT_RELU, _lib.FIODE_ACT_GROUPSORT) == (RELU, GROUPSORT)


def _call(lib, _lib, cfg=None, dyn=None, G=None, ws_bytes=0, activation=0, null=None):
    p = ct.c_void_p(1)
    cfg = cfg or _lib.CrownConfig(10, 8, 61, 3, 0.141, 0.225, 0)
    dyn = dyn or _lib.DynConfig(10, 128, 10, 100.0, 20.0, 0.02, 1, 0.5, 30, 1e-4)
    w = _lib.DynWeights(*[1] * 8)
    G = lib.fiode_certify_grid_rows(10, 8) if G is None else G
    a = dict(x_feat=p, grid=p, out=p, workspace=p)
    if null:
        a[null] = None
    return lib.fiode_certify_crown_act(None, ct.byref(cfg), ct.byref(dyn), ct.byref(w), a["x_feat"], a["grid"], G,
                                       a["out"], None, None, None, a["workspace"], ws_bytes, activation)


@pytest.mark.parametrize("act", [RELU, GROUPSORT])
def test_arguments_are_checked_before_the_workspace(act):
    """The table of tests/test_crown_abi.py for both activations: dummy non-NULL pointers and a zero-byte
    workspace, so a valid call reaches the workspace check (nothing is launched) and every bad argument
    returns its own code first."""
    from fiode_amd import _lib
    lib = _lib.lib()
    C = _lib.CrownConfig
    call = lambda **kw: _call(lib, _lib, activation=act, **kw)
    assert call() == EWORKSPACE
    assert _call(lib, _lib, activation=2) == EINVAL and _call(lib, _lib, activation=-1) == EINVAL
    for null in ("x_feat", "grid", "out", "workspace"):
        assert call(null=null) == EINVAL, null
    assert call(cfg=C(9, 8, 61, 3, 0.141, 0.225, 0)) == ESHAPE
    assert call(dyn=_lib.DynConfig(10, 64, 10, 100.0, 20.0, 0.02, 1, 0.5, 30, 1e-4)) == ESHAPE
    assert call(dyn=_lib.DynConfig(10, 128, 10, 100.0, 20.0, 0.02, 1, 0.5, 33, 1e-4)) == EINVAL
    for bad in (C(10, 8, 61, 10, 0.141, 0.225, 0), C(10, 8, 61, -1, 0.141, 0.225, 0), C(10, 0, 61, 3, 0.141, 0.225, 0),
                C(10, 65, 61, 3, 0.141, 0.225, 0), C(10, 8, 0, 3, 0.141, 0.225, 0), C(10, 8, 61, 3, 0.141, 0.0, 0)):
        assert call(cfg=bad) == EINVAL, [getattr(bad, f) for f, _ in bad._fields_]
    assert call(G=60) == EINVAL and call(G=1 << 32) == EINVAL                # G < batches, G >= 2^32
    assert call(G=-1) == EINVAL
    assert call(cfg=C(10, 8, 61, 3, -5.0, 0.225, 1)) == EWORKSPACE            # eps is only an offset
    assert call(G=0) == 0                                                    # a no-op


def test_workspace_is_batch_rows_plus_the_fixed_folded_images():
    from fiode_amd import _lib
    lib = _lib.lib()
    size = lib.fiode_certify_crown_workspace_bytes_act
    G8, G40 = lib.fiode_certify_grid_rows(10, 8), lib.fiode_certify_grid_rows(10, 40)
    # the folded images: A1, F2, H3, N3 [10][64], M2 [64][64], G3 [10][10] and a few vectors: under 32 KiB,
    # and the same for every grid; nothing of the size of G
    extra = size(G8, 61, GROUPSORT) - size(G8, 61, RELU)
    assert (4 * 640 + 4096 + 100) * 4 <= extra <= 32768
    assert size(G40, 400, GROUPSORT) - size(G40, 400, RELU) == extra
    assert size(G8, 1, GROUPSORT) - size(G8, 1, RELU) == extra
    for G, b in ((G8, 61), (G40, 400), (G8, 1)):
        assert size(G, b, RELU) == lib.fiode_certify_crown_workspace_bytes(G, b)
    need = size(G8, 61, GROUPSORT)
    assert _call(lib, _lib, ws_bytes=need - 1, activation=GROUPSORT) == EWORKSPACE
    assert _call(lib, _lib, ws_bytes=size(G8, 61, RELU) - 1, activation=RELU) == EWORKSPACE
    assert size(0, 61, GROUPSORT) == 256 and size(G8, 0, GROUPSORT) == 256 and size(G8, 61, 2) == 256


def test_fiode_certify_crown_still_refuses_groupsort():
    from fiode_amd import _lib
    lib = _lib.lib()
    p = ct.c_void_p(1)
    cfg = _lib.CrownConfig(10, 8, 61, 3, 0.141, 0.225, 0)
    dyn = _lib.DynConfig(10, 128, 10, 100.0, 20.0, 0.02, 1, 0.5, 30, 1e-4)
    w = _lib.DynWeights(*[1] * 8)
    G = lib.fiode_certify_grid_rows(10, 8)
    assert lib.fiode_certify_crown(None, ct.byref(cfg), ct.byref(dyn), ct.byref(w), p, p, G, p, None, None, None, p, 0,
                                   GROUPSORT) == ESHAPE


def _wrapper(ops):
    return ops.certify_crown_image(torch.zeros(10), 1, torch.zeros((423, 10), dtype=torch.uint8), {},
                                   ops.DynCfg(activation="GroupSort"), T=6, batches=10)


def test_switch_off_refuses_on_passes_the_refusal_and_is_restored():
    """Host tensors.  Off (the default): the refusal of tests/test_crown_abi.py.  On: the wrapper gets past
    it and fails on the device check of its tensors; certify_crown gets past its own.  The switch is back
    after the exception."""
    from fiode_amd import ops
    from fiode_amd.certify import certify_crown
    from tests.test_groupsort_dyn import build_module
    assert ops.GROUPSORT_CROWN is False
    with pytest.raises(NotImplementedError, match="ReLU"):
        _wrapper(ops)
    with pytest.raises(ValueError, match="ROCm device"):
        with ops.groupsort_crown():
            assert ops.GROUPSORT_CROWN is True
            _wrapper(ops)
    assert ops.GROUPSORT_CROWN is False
    with ops.groupsort_crown():
        with ops.groupsort_crown(False):
            with pytest.raises(NotImplementedError, match="ReLU"):
                _wrapper(ops)
        assert ops.GROUPSORT_CROWN is True
    assert ops.GROUPSORT_CROWN is False
    mod = build_module("GroupSort")
    args = (mod, torch.rand(1, 3, 32, 32), torch.tensor([1]))
    with pytest.raises(NotImplementedError, match="ReLU"):
        certify_crown(*args, T=6, batches=10)
    with pytest.raises(Exception) as e:                       # past the refusal: host tensors have no stream
        with ops.groupsort_crown():
            certify_crown(*args, T=6, batches=10, grid=torch.zeros((423, 10), dtype=torch.uint8))
    assert not isinstance(e.value, NotImplementedError), e.value
    assert ops.GROUPSORT_CROWN is False
    # an activation that is neither stays refused with the switch on
    with ops.groupsort_crown():
        with pytest.raises(ValueError, match="activation"):
            ops.certify_crown_image(torch.zeros(10), 1, torch.zeros((423, 10), dtype=torch.uint8), {},
                                    ops.DynCfg(activation="Tanh"), T=6, batches=10)
