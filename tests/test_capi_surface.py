"""CPU, without the library: the public surface of cvr_amd/capi.py against tests/golden/capi_surface.json -- every public module-level function and
every public method, classmethod and property (and __init__) of Precond, CvrMatrix, SpGemm, Comm and MultiMatrix: the kind of callable,
str(inspect.signature(...)) and the docstring.  The fixture was written by `PYTHONPATH=. python tests/test_capi_surface.py` from the module as it stood before
its builders and solver calls were folded into shared helpers; run that again only when the surface is meant to change."""
import inspect
import json
import os

from cvr_amd import capi

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "capi_surface.json")
CLASSES = ["Precond", "CvrMatrix", "SpGemm", "Comm", "MultiMatrix"]


def _entry(kind, fn):
    return {"kind": kind, "signature": str(inspect.signature(fn)), "doc": fn.__doc__}


def _member(raw):
    if isinstance(raw, classmethod):
        return _entry("classmethod", raw.__func__)
    if isinstance(raw, staticmethod):
        return _entry("staticmethod", raw.__func__)
    if isinstance(raw, property):
        return _entry("property", raw.fget)
    if inspect.isfunction(raw):
        return _entry("method", raw)
    return None


def surface():
    functions = {name: _entry("function", f) for name, f in vars(capi).items()
                 if not name.startswith("_") and inspect.isfunction(f) and f.__module__ == capi.__name__}
    classes = {}
    for cname in CLASSES:
        members = {name: _member(raw) for name, raw in vars(getattr(capi, cname)).items() if name == "__init__" or not name.startswith("_")}
        classes[cname] = {name: m for name, m in members.items() if m is not None}
    return {"functions": functions, "classes": classes}


def _flat(s):
    out = {("capi", name): e for name, e in s["functions"].items()}
    for cname, members in s["classes"].items():
        out.update({(cname, name): e for name, e in members.items()})
    return out


def test_the_public_surface_is_the_recorded_one():
    with open(FIXTURE) as f:
        want = _flat(json.load(f))
    got = _flat(surface())
    assert sorted(got) == sorted(want), (sorted(set(want) - set(got)), sorted(set(got) - set(want)))          # (missing, new)
    changed = {".".join(k): [f for f in ("kind", "signature", "doc") if got[k][f] != want[k][f]] for k in want if got[k] != want[k]}
    assert not changed, changed
    assert len(want) >= 136 and("Precond", "amg_block_from_device") in want and ("CvrMatrix", "lsqr_host") in want and ("capi", "amg_setup_host") in want


if __name__ == "__main__":
    with open(FIXTURE, "w") as f:
        json.dump(surface(), f, indent=1, sort_keys=True)
        f.write("\n")
    print(FIXTURE, len(_flat(surface())), "entries")
