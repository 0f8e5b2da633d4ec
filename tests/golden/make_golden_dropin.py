"""Generates tests/golden/dropin_reference.npz from the reference's own files (build container only):

    python tests/golden/make_golden_dropin.py <reference checkout>

What tests/test_dropin_fixtures.py holds the drop-in modules against, so that it runs without the reference tree:

  meta (a JSON string)
    backends.<pkg>.used    the `_backend.<fn>(` calls of aux_libs/raymarching/raymarching.py and
                           aux_libs/shencoder/sphere_harmonics.py (names only)
    backends.<pkg>.arity   per function of src/raymarching.h / src/shencoder.h its number of parameters
    ffmlp.<args>           num_parameters, repr, state-dict keys, padded_output_dim, activation, output_activation of
                           the reference's aux_libs/ffmlp/ffmlp.py FFMLP(*args), constructed with its CUDA backend
                           replaced by an empty stand-in (only `allocate_splitk` is touched at construction)
  ffmlp/<args>/weights     that module's initial weights (`manual_seed(42)` + uniform on the host)

Nothing of the source text is stored -- only names, counts and the values the reference's code produces.
"""
import importlib.util
import json
import os
import re
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
BACKENDS = (("raymarching", "raymarching.py", "src/raymarching.h"), ("shencoder", "sphere_harmonics.py", "src/shencoder.h"))
FFMLP_ARGS = ((48, 16, 64, 2), (32, 3, 64, 3), (144, 16, 128, 2), (32, 3, 128, 3))


def header_arity(path):
    txt = open(path).read()
    return {m.group(1): len([a for a in m.group(2).split(",") if a.strip()])
            for m in re.finditer(r"void\s+(\w+)\s*\(([^;]*)\)\s*;", txt)}


def main(ref):
    aux = os.path.join(ref, "aux_libs")
    meta = {"backends": {}, "ffmlp": {}}
    for pkg, fname, hdr in BACKENDS:
        used = sorted(set(re.findall(r"_backend\.(\w+)\(", open(os.path.join(aux, pkg, fname)).read())))
        meta["backends"][pkg] = {"used": used, "arity": header_arity(os.path.join(aux, pkg, hdr))}
    be = types.ModuleType("_ffmlp")
    be.allocate_splitk = lambda n: None
    be.free_splitk = lambda: None
    sys.modules["_ffmlp"] = be
    tu = types.ModuleType("turtle")          # ffmlp.py:2 (a stray import; needs tkinter)
    tu.backward = tu.forward = None
    sys.modules["turtle"] = tu
    spec = importlib.util.spec_from_file_location("ref_ffmlp", os.path.join(aux, "ffmlp", "ffmlp.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    arrays = {}
    for args in FFMLP_ARGS:
        m = mod.FFMLP(*args)
        key = ",".join(map(str, args))
        meta["ffmlp"][key] = {"num_parameters": m.num_parameters, "repr": repr(m), "state_dict": list(m.state_dict()),
                              "padded_output_dim": m.padded_output_dim, "activation": m.activation,
                              "output_activation": m.output_activation}
        arrays[f"ffmlp/{key}/weights"] = m.weights.detach().numpy().astype(np.float32)
    out = os.path.join(HERE, "dropin_reference.npz")
    np.savez_compressed(out, meta=np.array(json.dumps(meta, sort_keys=True)), **arrays)
    print(out, json.dumps(meta["backends"]))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
