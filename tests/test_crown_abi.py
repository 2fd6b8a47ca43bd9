"""CPU checks of the CROWN certification entry points (include/fiode.h, crown.hip): declared, exported,
arguments checked on the host before the workspace and before any launch."""
import ctypes as ct
import pathlib
import re

import pytest
import torch

ROOT = pathlib.Path(__file__).resolve().parents[1]
SYMBOLS = ("fiode_certify_crown", "fiode_certify_crown_workspace_bytes")
EINVAL, ESHAPE, EWORKSPACE = 1, 2, 3


def test_header_declares_and_library_exports_the_crown_symbols():
    from fiode_amd import _lib
    text = (ROOT / "include" / "fiode.h").read_text()
    declared = re.findall(r"FIODE_API\s+[\w\s\*]+?\b(fiode_\w+)\s*\(", text)
    lib = ct.CDLL(str(_lib.LIB_PATH))
    for s in SYMBOLS:
        assert s in declared and hasattr(lib, s), s
    assert "typedef struct fiode_crown_config" in text and "typedef struct fiode_crown_debug" in text
    assert _lib.lib().fiode_abi_version() == _lib.ABI_VERSION == 5           # new symbols only
    assert ct.sizeof(_lib.CrownConfig) == 28 and ct.sizeof(_lib.CrownDebug) == 6 * ct.sizeof(ct.c_void_p)


def _call(lib, _lib, cfg=None, dyn=None, G=None, ws_bytes=0, activation=0, null=None):
    p = ct.c_void_p(1)
    cfg = cfg or _lib.CrownConfig(10, 8, 61, 3, 0.141, 0.225, 0)
    dyn = dyn or _lib.DynConfig(10, 128, 10, 100.0, 20.0, 0.02, 1, 0.5, 30, 1e-4)
    w = _lib.DynWeights(*[1] * 8)
    G = lib.fiode_certify_grid_rows(10, 8) if G is None else G
    a = dict(x_feat=p, grid=p, out=p, workspace=p)
    if null:
        a[null] = None
    return lib.fiode_certify_crown(None, ct.byref(cfg), ct.byref(dyn), ct.byref(w), a["x_feat"], a["grid"], G, a["out"],
                                   None, None, None, a["workspace"], ws_bytes, activation)


def test_arguments_are_checked_before_the_workspace():
    """Dummy non-NULL pointers and a zero-byte workspace: a valid call reaches the workspace check
    (nothing is launched), every bad argument returns its own code first."""
    from fiode_amd import _lib
    lib = _lib.lib()
    C = _lib.CrownConfig
    assert _call(lib, _lib) == EWORKSPACE
    assert _call(lib, _lib, activation=1) == ESHAPE                      # GroupSort: unsupported
    assert _call(lib, _lib, activation=2) == EINVAL and _call(lib, _lib, activation=-1) == EINVAL
    for null in ("x_feat", "grid", "out", "workspace"):
        assert _call(lib, _lib, null=null) == EINVAL, null
    assert _call(lib, _lib, cfg=C(9, 8, 61, 3, 0.141, 0.225, 0)) == ESHAPE
    assert _call(lib, _lib, dyn=_lib.DynConfig(10, 64, 10, 100.0, 20.0, 0.02, 1, 0.5, 30, 1e-4)) == ESHAPE
    assert _call(lib, _lib, dyn=_lib.DynConfig(10, 128, 10, 100.0, 20.0, 0.02, 1, 0.5, 33, 1e-4)) == EINVAL
    for bad in (C(10, 8, 61, 10, 0.141, 0.225, 0), C(10, 8, 61, -1, 0.141, 0.225, 0), C(10, 0, 61, 3, 0.141, 0.225, 0),
                C(10, 65, 61, 3, 0.141, 0.225, 0), C(10, 8, 0, 3, 0.141, 0.225, 0), C(10, 8, 61, 3, 0.141, 0.0, 0)):
        assert _call(lib, _lib, cfg=bad) == EINVAL, [getattr(bad, f) for f, _ in bad._fields_]
    assert _call(lib, _lib, G=60) == EINVAL and _call(lib, _lib, G=1 << 32) == EINVAL      # G < batches, G >= 2^32
    assert _call(lib, _lib, G=-1) == EINVAL
    assert _call(lib, _lib, cfg=C(10, 8, 61, 3, -5.0, 0.225, 1)) == EWORKSPACE              # eps is only an offset


def test_zero_rows_is_a_no_op_and_workspace_size():
    from fiode_amd import _lib
    lib = _lib.lib()
    assert _call(lib, _lib, G=0) == 0
    G = lib.fiode_certify_grid_rows(10, 8)
    need = lib.fiode_certify_crown_workspace_bytes(G, 61)
    # [largest batch = 30 rows][20] floats, u, r1, three words per batch: O(batch rows), not O(G)
    assert 30 * 20 * 4 <= need <= 8192
    assert _call(lib, _lib, ws_bytes=need - 1) == EWORKSPACE
    assert lib.fiode_certify_crown_workspace_bytes(0, 61) == 256 and lib.fiode_certify_crown_workspace_bytes(G, 0) == 256
    G40 = lib.fiode_certify_grid_rows(10, 40)
    rows = G40 // 400 + G40 % 400
    assert lib.fiode_certify_crown_workspace_bytes(G40, 400) <= max(rows, G40 // 400) * 128 * 4


def test_groupsort_refuses_before_anything_is_launched():
    """Host tensors: certify_crown and the wrapper refuse a GroupSort dynamics before any device work."""
    from fiode_amd import ops
    from fiode_amd.certify import certify_crown
    from tests.test_groupsort_dyn import build_module
    mod = build_module("GroupSort")
    with pytest.raises(NotImplementedError, match="ReLU"):
        certify_crown(mod, torch.rand(1, 3, 32, 32), torch.tensor([1]), T=6, batches=10)
    with pytest.raises(NotImplementedError, match="ReLU"):
        ops.certify_crown_image(torch.zeros(10), 1, torch.zeros((423, 10), dtype=torch.uint8), {},
                                ops.DynCfg(activation="GroupSort"), T=6, batches=10)
