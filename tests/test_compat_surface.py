"""The surface of image_search_engine_amd.faiss_compat, pinned: every name the module defines, every signature, every
class attribute and every base recorded in tests/golden/faiss_compat_surface.json still exists with the same signature
or kind.  New private names and new intermediate bases are allowed; nothing recorded may go or change (no GPU needed).

The fixture was written by ``describe_surface`` below, from the module as it stood before its index kinds began to
share their Python code:  python -m tests.test_compat_surface > tests/golden/faiss_compat_surface.json
``gemm_stats`` of the flat index kinds, a reader added since, was recorded in it from the same function's output.

A second fixture, tests/golden/faiss_compat_surface_coded.json, holds the 16 public names of the kinds that came after
the first was recorded (``_CODED`` below), with the attributes of a class that do not start with ``_`` plus ``__init__``
and ``__del__``.  It was written from the module as it stood before the coded and inverted-list kinds shared their
Python code:  python -m tests.test_compat_surface coded > tests/golden/faiss_compat_surface_coded.json"""
import inspect
import json
import os
import types

from image_search_engine_amd import faiss_compat

_KEPT_DUNDERS = ("__init__", "__del__")


def _describe_attr(obj) -> str:
    if isinstance(obj, (staticmethod, classmethod)):
        obj = obj.__func__
    if isinstance(obj, property):
        return "property"
    if inspect.isfunction(obj):
        return str(inspect.signature(obj))
    return type(obj).__name__


def _describe_class(cls) -> dict:
    attrs = {}
    for name in dir(cls):
        if name.startswith("__") and name.endswith("__") and name not in _KEPT_DUNDERS:
            continue
        attrs[name] = _describe_attr(inspect.getattr_static(cls, name))
    bases = [b.__name__ for b in cls.__mro__[1:] if b.__module__ == faiss_compat.__name__]
    return {"kind": "class", "bases": bases, "attrs": attrs}


def describe_surface(module=faiss_compat) -> dict:
    """name -> description, for every name ``module`` itself defines (imports and dunder names are not its own)."""
    out = {}
    for name, obj in sorted(vars(module).items()):
        if name.startswith("__") and name.endswith("__"):
            continue
        if isinstance(obj, types.ModuleType):
            continue
        if inspect.isclass(obj) or inspect.isfunction(obj):
            if obj.__module__ != module.__name__:
                continue
            out[name] = _describe_class(obj) if inspect.isclass(obj) else \
                {"kind": "function", "signature": str(inspect.signature(obj))}
        else:
            entry = {"kind": "value", "type": type(obj).__name__}
            if name in ("_HDR", "_BHDR"):
                entry["format"] = obj.format
            out[name] = entry
    return out


_CODED = ("IndexPQ", "IndexScalarQuantizer", "IndexIVFScalarQuantizer", "IndexRefine", "IndexRefineFlat",
          "IndexRefineSearchParameters", "ProductQuantizer", "ScalarQuantizer", "serialize_pq", "parse_pq", "serialize_sq",
          "parse_sq", "serialize_ivfsq", "parse_ivfsq", "serialize_refine", "parse_refine")


def describe_coded_surface() -> dict:
    """``describe_surface`` of the names in ``_CODED``, without the private attributes of the classes."""
    out = {name: desc for name, desc in describe_surface().items() if name in _CODED}
    for desc in out.values():
        if desc["kind"] == "class":
            desc["attrs"] = {a: v for a, v in desc["attrs"].items() if not a.startswith("_") or a in _KEPT_DUNDERS}
    return out


def _problems(recorded: dict, now: dict) -> list:
    problems = []
    for name, want in recorded.items():
        got = now.get(name)
        if got is None:
            problems.append(f"{name}: gone")
            continue
        if want["kind"] != "class":
            if got != want:
                problems.append(f"{name}: {want} became {got}")
            continue
        if got["kind"] != "class":
            problems.append(f"{name}: a class became {got}")
            continue
        for base in want["bases"]:
            if base not in got["bases"]:
                problems.append(f"{name}: base {base} left the MRO")
        for attr, desc in want["attrs"].items():
            if got["attrs"].get(attr) != desc:
                problems.append(f"{name}.{attr}: {desc!r} became {got['attrs'].get(attr)!r}")
    return problems


def test_nothing_recorded_has_gone_or_changed(golden_dir):
    with open(os.path.join(golden_dir, "faiss_compat_surface.json")) as f:
        recorded = json.load(f)
    assert len(recorded) >= 54
    problems = _problems(recorded, describe_surface())
    assert not problems, "\n".join(problems)


def test_nothing_recorded_of_the_coded_kinds_has_gone_or_changed(golden_dir):
    with open(os.path.join(golden_dir, "faiss_compat_surface_coded.json")) as f:
        recorded = json.load(f)
    assert sorted(recorded) == sorted(_CODED)
    problems = _problems(recorded, describe_coded_surface())
    assert not problems, "\n".join(problems)


if __name__ == "__main__":
    import sys

    surface = describe_coded_surface() if sys.argv[1:] == ["coded"] else describe_surface()
    print(json.dumps(surface, indent=1, sort_keys=True))
