"""The drop-in boundary against what the reference's own files declare and produce, stored in
tests/golden/dropin_reference.npz (tests/golden/make_golden_dropin.py): the native names the reference's wrapper files
call with their parameter counts, and the reference FFMLP's shapes, repr and initial weights.  The same checks against
the live reference tree are in test_dropin_reference.py, which runs only where that tree exists.  Every check runs in a
child process: install_dropin() / install_backends() rewire sys.modules / sys.path."""
import json
import os
import subprocess
import sys
import textwrap

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "dropin_reference.npz")


def _meta():
    return json.loads(str(np.load(GOLDEN)["meta"]))


def _run(body):
    prelude = f"import json, os, sys, types\nsys.path.insert(0, {ROOT!r})\nGOLDEN = {GOLDEN!r}\n"
    r = subprocess.run([sys.executable, "-c", prelude + textwrap.dedent(body)], capture_output=True, text=True, timeout=600,
                       cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_backends_bind_the_native_names_the_reference_wrappers_call():
    """aux_libs/raymarching/raymarching.py and aux_libs/shencoder/sphere_harmonics.py do `import _raymarching as _backend`
    / `import _shencoder as _backend`; with install_backends() these are this build's modules, and every
    `_backend.<fn>(...)` call of the reference's wrapper files names a function here with the parameter count of the
    reference's prototype (raymarching.h / shencoder.h)."""
    meta = _meta()["backends"]
    assert meta["raymarching"]["used"] == ["composite_rays", "composite_rays_train_backward", "composite_rays_train_forward",
                                           "march_rays", "march_rays_train", "morton3D", "morton3D_invert",
                                           "near_far_from_aabb", "packbits", "sph_from_ray"]
    assert meta["shencoder"]["used"] == ["sh_encode_backward", "sh_encode_forward"]
    out = _run("""
        import inspect
        import numpy as np
        import trinerflet_amd
        trinerflet_amd.install_backends()
        meta = json.loads(str(np.load(GOLDEN)["meta"]))["backends"]
        for pkg, native in (("raymarching", "_raymarching"), ("shencoder", "_shencoder")):
            be = __import__(native)
            assert be.__name__ == native and "/trinerflet_amd/backends/" in be.__file__, be
            used, arity = set(meta[pkg]["used"]), meta[pkg]["arity"]
            assert used <= set(arity), (used, arity)
            for fn, n in arity.items():
                assert len(inspect.signature(getattr(be, fn)).parameters) == n, (fn, n)
            print(native, sorted(arity))
        print("BACKENDS_OK")
    """)
    assert "BACKENDS_OK" in out
    assert "_raymarching ['composite_rays', 'composite_rays_train_backward', 'composite_rays_train_forward', " \
           "'march_rays', 'march_rays_train', 'morton3D', 'morton3D_invert', 'near_far_from_aabb', 'packbits', " \
           "'sph_from_ray']" in out


def test_ff_switch_constructs_the_reference_shapes_and_its_initial_weights():
    """`--ff` (main_nerf.py:31-34: `from nerf.network_ff import NeRFNetwork`, network_ff.py:7 `from ffmlp import FFMLP`).
    After install_dropin() both names resolve to this build.  Pinned against the reference FFMLP's recorded construction:
    the same parameter count, state-dict key, repr, padding and activations, and -- the initialisation is `manual_seed(42)`
    + uniform on the host -- the same initial weights to the bit, for both networks of the `--ff` model."""
    assert set(_meta()["ffmlp"]) == {"48,16,64,2", "32,3,64,3", "144,16,128,2", "32,3,128,3"}
    out = _run("""
        import numpy as np
        import torch
        import trinerflet_amd
        trinerflet_amd.install_dropin()
        import ffmlp, nerf.network_ff as nff
        assert "/trinerflet_amd/" in ffmlp.__file__ and "/trinerflet_amd/" in nff.__file__
        z = np.load(GOLDEN)
        meta = json.loads(str(z["meta"]))["ffmlp"]
        for key, ref in meta.items():
            b = ffmlp.FFMLP(*map(int, key.split(",")))
            assert b.num_parameters == ref["num_parameters"] and repr(b) == ref["repr"], (repr(b), ref)
            assert list(b.state_dict()) == ref["state_dict"] == ["weights"]
            assert (b.padded_output_dim, b.activation, b.output_activation) == \\
                (ref["padded_output_dim"], ref["activation"], ref["output_activation"])
            w = z[f"ffmlp/{key}/weights"]
            assert b.weights.dtype == torch.float32 and np.array_equal(b.weights.detach().numpy(), w), key
        m = nff.NeRFNetwork(encoding="triplane_wavelet", bound=1.5, cuda_ray=True, density_scale=1, min_near=0.2,
                            density_thresh=10, bg_radius=-1, triplane_channels=16, triplane_resolution=64,
                            triplane_wavelet_levels=1, wavelet_type="bior6.8", hidden_dim=64, hidden_dim_color=64)
        keys = set(m.state_dict())
        assert {"sigma_net.weights", "color_net.weights", "encoder.planes_features", "density_grid", "density_bitfield"} <= keys
        assert m.in_dim == 48 and m.in_dim_color == 32 and len(m.get_params(1e-2)) == 4
        print("FF_OK")
    """)
    assert "FF_OK" in out
