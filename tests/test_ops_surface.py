"""``deformcontact_amd.ops`` is the package's public operator surface and the home of every run-time switch, whichever
module holds the code.  ``tests/golden/ops_surface.json`` is ``record(ops)`` of the commit BEFORE the layer operators
moved to ``deformcontact_amd/layers/`` (``python tests/test_ops_surface.py > tests/golden/ops_surface.json`` there):

* ``functions``: every function in ``dir(ops)`` without a leading underscore that ``ops.py`` defined, with its
  ``__doc__`` and ``str(inspect.signature(...))``;
* ``others``: the public classes and instances it defined (``OutInto``, ``SIX_PRODUCTS``);
* ``constants``: the upper-case module-level values nobody sets (kernel caps, mode tables);
* ``switches``: the upper-case module-level names that code reads at call time and users, tests and ``bench.py`` set
  through ``ops.`` - a switch defined in another module and imported into ``ops`` would be a copy that setting
  ``ops.NAME`` no longer reaches, without any error.
"""
import importlib
import inspect
import json
import os
import pkgutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def record(ops):
    out = {"functions": {}, "others": [], "constants": {}, "switches": []}
    for n in sorted(vars(ops)):
        obj = getattr(ops, n)
        if n.startswith("_") or inspect.ismodule(obj):
            continue
        if inspect.isfunction(obj):
            if obj.__module__ == ops.__name__:
                out["functions"][n] = {"doc": obj.__doc__, "signature": str(inspect.signature(obj))}
        elif getattr(obj, "__module__", None) == ops.__name__:
            out["others"].append(n)
        elif n.isupper():
            if obj is None or isinstance(obj, bool) or n in ("DENSE_PRODUCTS", "DW_POSITION", "DW_LAST_STREAMS"):
                out["switches"].append(n)
            else:
                out["constants"][n] = obj
    return out


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from deformcontact_amd import ops as _ops
    json.dump(record(_ops), sys.stdout, indent=1)
    sys.exit(0)


from deformcontact_amd import _host, layers, ops  # noqa: E402

LAYERS = sorted(m.name for m in pkgutil.iter_modules(layers.__path__))
LAYER_MODULES = [importlib.import_module(f"deformcontact_amd.layers.{m}") for m in LAYERS]


@pytest.fixture(scope="module")
def surface(golden_dir):
    with open(os.path.join(golden_dir, "ops_surface.json")) as f:
        return json.load(f)


def test_public_names(surface):
    assert len(surface["functions"]) >= 44 and surface["others"] and surface["constants"]
    for n in list(surface["functions"]) + surface["others"] + list(surface["constants"]) + surface["switches"]:
        assert hasattr(ops, n), f"ops.{n} no longer resolves"
    for n, was in surface["functions"].items():
        f = getattr(ops, n)
        home = sys.modules[f.__module__]
        assert home is ops or home in LAYER_MODULES, f"ops.{n} lives in {f.__module__}"
        assert getattr(home, n) is f
        assert f.__doc__ == was["doc"], f"ops.{n}: docstring changed"
        assert str(inspect.signature(f)) == was["signature"], f"ops.{n}: signature changed"
    for n in surface["others"]:
        assert getattr(ops, n).__module__ == ops.__name__, f"ops.{n} moved"
    for n, was in surface["constants"].items():
        value = getattr(ops, n)
        assert json.loads(json.dumps(value)) == was, f"ops.{n} changed"
        homes = [m for m in [ops] + LAYER_MODULES if n in vars(m)]
        assert all(vars(m)[n] is value for m in homes), f"{n} is more than one object"


def test_switches_live_in_ops(surface):
    assert {"HOP_CHAIN", "DENSE_SPLIT_BF16", "FUSED_GNN_EPILOGUE", "POINTNET_PAD_Z"} <= set(surface["switches"])
    for n in surface["switches"]:
        assert n in vars(ops), f"the switch {n} left ops.py"
        for m in LAYER_MODULES + [_host]:
            assert n not in vars(m), f"{m.__name__}.{n} is a copy that setting ops.{n} does not reach"


@pytest.mark.parametrize("name", LAYERS)
def test_layer_module_imports_first(name):
    """A layer module imports ``ops`` and ``ops`` re-exports from it: the cycle must resolve whichever a process asks
    for first."""
    r = subprocess.run([sys.executable, "-c", f"import deformcontact_amd.layers.{name}"], cwd=ROOT,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.gpu
def test_moved_switches_take_effect(monkeypatch):
    """The two switches whose readers moved out of ``ops.py`` are still read through ``ops.`` at call time."""
    import torch
    from deformcontact_amd.layers import gnn
    dev = torch.device("cuda:0")
    h = torch.zeros(8, 16, device=dev)
    assert ops.fused_gnn_ok(h) and gnn.fused_gnn_ok(h)
    with monkeypatch.context() as mp:
        mp.setattr(ops, "FUSED_GNN_EPILOGUE", False)
        assert not ops.fused_gnn_ok(h) and not gnn.fused_gnn_ok(h)

    ei = torch.tensor([[0, 1, 2], [1, 2, 3]], device=dev)
    g = ops.pointnet_graph(ei, 4, 4)
    x, pos = torch.randn(4, 4, device=dev), torch.randn(4, 3, device=dev)
    z = ops.pointnet_pairs(g, x, pos, pos)
    assert z.shape == (3, 7) and z.stride() == (8, 1)
    monkeypatch.setattr(ops, "POINTNET_PAD_Z", False)
    zc = ops.pointnet_pairs(g, x, pos, pos)
    assert zc.shape == (3, 7) and zc.stride() == (7, 1) and zc.is_contiguous()
    assert torch.equal(z, zc)
