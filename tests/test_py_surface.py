"""The Python binding's public surface (CPU only): the attribute names and call shapes of the public
classes and the module's constants, dtypes and structures, against tests/golden/py_surface.json
(written once by `python tests/test_py_surface.py` and kept)."""
import ctypes as C
import inspect
import json
import os

import numpy as np

import crdt_hip

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "py_surface.json")
CLASSES = ["OpLog", "Replica", "Context", "Batch", "UpdateBatch", "Mark", "Trace", "LogFile", "HipMerge",
           "HipDownstream", "HipDownstreamBytes"]


def _shape(fn) -> str:
    """The call shape: parameter names, kinds and defaults.  Annotations are left out (a method
    shared by two classes cannot name either as the type of its peer)."""
    sig = inspect.signature(fn)
    return str(sig.replace(parameters=[p.replace(annotation=p.empty) for p in sig.parameters.values()],
                           return_annotation=sig.empty))


def _member(cls, name) -> str:
    static = inspect.getattr_static(cls, name)
    if isinstance(static, property):
        return "property"
    value = getattr(cls, name)
    if callable(value):
        kind = {staticmethod: "staticmethod ", classmethod: "classmethod "}.get(type(static), "")
        return kind + _shape(value)
    return "= " + repr(value)


def surface() -> dict:
    classes = {}
    for cname in CLASSES:
        cls = getattr(crdt_hip, cname)
        names = ["__init__"] + sorted(n for n in dir(cls) if not n.startswith("_"))
        classes[cname] = {n: _member(cls, n) for n in names}
    consts, dtypes, structs = {}, {}, {}
    for name, v in vars(crdt_hip).items():
        if name.startswith("_") or name in ("PKG_DIR", "LIB_PATH"):
            continue
        if isinstance(v, np.dtype):
            dtypes[name] = str(v.descr)
        elif isinstance(v, type) and issubclass(v, C.Structure):
            structs[name] = [[f, t.__name__] for f, t in v._fields_]
        elif isinstance(v, (int, str)):
            consts[name] = v
        elif isinstance(v, dict):
            consts[name] = {str(k): x for k, x in v.items()}
        elif isinstance(v, list):
            consts[name] = v if name != "EXPORTS" else sorted(v)
    return {"names": sorted(n for n in vars(crdt_hip) if not n.startswith("_")), "classes": classes,
            "constants": consts, "dtypes": dtypes, "structures": structs}


def test_python_surface_is_the_recorded_one():
    with open(GOLDEN) as f:
        want = json.load(f)
    got = json.loads(json.dumps(surface()))
    for part in want:
        if isinstance(want[part], dict):
            for k in sorted(set(want[part]) | set(got[part])):
                assert got[part].get(k) == want[part].get(k), (part, k)
        assert got[part] == want[part], part


if __name__ == "__main__":
    with open(GOLDEN, "w") as f:
        json.dump(surface(), f, indent=1, sort_keys=True)
        f.write("\n")
