"""Build-container-only check of the drop-in boundary against the reference's OWN files: after
trinerflet_amd.install_dropin() the import block of reconstruction/main_nerf.py:1-16,40 runs, the reference's
`nerf.utils` / `nerf.provider` keep coming from /root/reference while `nerf.network` / `nerf.renderer`, `raymarching`,
`shencoder`, `encoding`, `triplaneencoder` resolve to this build, the model is constructed exactly as main_nerf.py:44-72
does from the README's command lines, the reference's Trainer accepts it, and the reference's own
aux_libs/raymarching/raymarching.py / shencoder/sphere_harmonics.py bind `_raymarching` / `_shencoder` unchanged.

Skipped where /root/reference does not exist (the GPU box, a clean checkout); the wrapper-binding and `--ff` checks run
everywhere against recorded reference data in test_dropin_fixtures.py.  Every check runs in a child process: it rewires
sys.modules / sys.path.  Third-party packages the reference imports at module level but that this image lacks (cv2,
tensorboardX, mcubes, ...) are replaced by empty placeholder modules -- none is touched by the code under test."""
import os
import subprocess
import sys
import textwrap

import pytest

REF = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(not os.path.isdir(REF), reason="the reference tree exists only in the build container")

PRELUDE = textwrap.dedent("""
    import os, sys, types
    sys.path.insert(0, "@ROOT@")
    import importlib.abc, importlib.machinery
    THIRD_PARTY = {"imageio", "tensorboardX", "cv2", "trimesh", "mcubes", "lpips", "torch_ema", "torchmetrics",
                   "torchvision", "matplotlib", "kornia", "PIL", "open3d", "plyfile", "nerfacc", "tinycudann", "clip",
                   "dearpygui", "pytorch_wavelets", "skimage", "pycolmap", "pytorch_lightning", "imageio_ffmpeg"}
    class _Anything:
        def __init__(self, *a, **k): pass
        def __call__(self, *a, **k): return _Anything()
        def __getattr__(self, n): return _Anything()
    class _Placeholder(types.ModuleType):
        __path__ = []
        def __getattr__(self, n):
            if n.startswith("__"):
                raise AttributeError(n)
            return _Anything
    class _Finder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
        # absent third-party packages only (never the reference's or this repo's modules)
        def find_spec(self, name, path=None, target=None):
            if name.split(".")[0] not in THIRD_PARTY:
                return None
            return importlib.machinery.ModuleSpec(name, self, is_package=True)
        def create_module(self, spec): return _Placeholder(spec.name)
        def exec_module(self, module): pass
    sys.meta_path.append(_Finder())      # last: anything really installed wins
    # `python main_nerf.py` puts the script directory first on sys.path
    sys.path.insert(0, "@REF@/reconstruction")
    os.chdir("@REF@/reconstruction")
    import trinerflet_amd
    trinerflet_amd.install_dropin()
""").replace("@ROOT@", ROOT).replace("@REF@", REF)

MAIN_NERF_BLOCK = textwrap.dedent("""
    # ---- reconstruction/main_nerf.py:1-16, verbatim order
    import torch
    import argparse
    from nerf.provider import NeRFDataset , get_dataset
    from nerf.utils import *
    from functools import partial
    from loss import huber_loss
    import copy
    import sys
    from run_utils import get_params
    import sys,os
    dir_path = os.path.dirname(os.path.dirname(os.path.realpath("main_nerf.py")))
    sys.path.append(os.path.join(dir_path,'aux_libs'))
    from nerf.network import NeRFNetwork                                    # main_nerf.py:40
""")


def _run(body, *argv):
    r = subprocess.run([sys.executable, "-c", PRELUDE + body, *argv], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_main_nerf_import_block_after_install_dropin():
    out = _run(MAIN_NERF_BLOCK + textwrap.dedent("""
        import nerf, nerf.utils, nerf.provider, nerf.network, nerf.renderer, raymarching, shencoder, encoding
        import triplaneencoder.triplane_encoder as te
        ref = "/root/reference/"
        assert nerf.utils.__file__.startswith(ref) and nerf.provider.__file__.startswith(ref)
        assert Trainer.__module__ == "nerf.utils" and NeRFDataset.__module__ == "nerf.provider"
        for m in (nerf.network, nerf.renderer, raymarching, shencoder, encoding, te):
            assert "/trinerflet_amd/" in m.__file__, m.__file__
        assert NeRFNetwork is trinerflet_amd.nerf.network.NeRFNetwork
        assert nerf.network is sys.modules["trinerflet_amd.nerf.network"]
        # the symbols the reference's renderer / encoding / trainer take from these modules
        for f in ("near_far_from_aabb", "sph_from_ray", "morton3D", "morton3D_invert", "packbits", "march_rays_train",
                  "composite_rays_train", "march_rays", "composite_rays"):
            assert callable(getattr(raymarching, f))
        from shencoder import SHEncoder
        from encoding import get_encoder
        # install_dropin() opts the encoders it will serve into the windowed rebuild under autograd (the reference's loop
        # discards get_planes()'s result); install_dropin(windowed_autograd=False) leaves whole planes
        assert te.WINDOWED_AUTOGRAD is True
        trinerflet_amd.install_dropin(windowed_autograd=False)
        assert te.WINDOWED_AUTOGRAD is False
        print("IMPORT_BLOCK_OK")
    """))
    assert "IMPORT_BLOCK_OK" in out


README_ARGS = {
    "small": "--fp16 --cuda_ray --bound 1.5 --scale 1 --dt_gamma 0 --iters 1000 5000 --num_rays 20000 60000 "
             "--background_color 0 --triplane_wavelet --triplane_channels 16 --triplane_wavelet_levels 8 16 "
             "--triplane_resolution 512 1024 --wavelet_regularization 0.2 --downscale 1 --ckpt latest_model "
             "--ema_decay -1 --training_evaluate_test --warmup_steps 0 200 --fast_training",
    "large": "--fp16 --cuda_ray --bound 1.5 --scale 1 --dt_gamma 0 --iters 1000 2000 80000 --num_rays 30000 60000 60000 "
             "--background_color 0 --triplane_wavelet --triplane_channels 48 --triplane_wavelet_levels 8 16 32 "
             "--triplane_resolution 512 1024 2048 --wavelet_regularization 0.6 --hidden_dim 128 --hidden_dim_color 128 "
             "--downscale 1 --ckpt latest_model --ema_decay -1 --training_evaluate_test --warmup_steps 0 100 1000",
}


@pytest.mark.parametrize("cfg", sorted(README_ARGS))
def test_model_and_reference_trainer_from_readme_command(cfg, tmp_path):
    """First stage of a README command line through the reference's get_params + the stage split of
    main_nerf.py:168-205, the model built as main_nerf.py:44-72, wrapped by the reference's Trainer (CPU device: the
    constructor, optimizer / scheduler wiring, get_params groups, state-dict save + reload)."""
    body = MAIN_NERF_BLOCK + textwrap.dedent(f"""
        sys.argv = ["main_nerf.py", "--path", "/nonexistent", "--workspace", {str(tmp_path)!r}] + {README_ARGS[cfg]!r}.split()
        opt = get_params()
        # main_nerf.py:172-205: list-valued flags are zipped into stages; take stage 0
        import copy
        stage = copy.deepcopy(opt)
        for k, v in vars(opt).items():
            if isinstance(v, list) and k in ("iters", "num_rays", "triplane_resolution", "triplane_wavelet_levels",
                                             "downscale", "warmup_steps", "lr", "wavelet_regularization",
                                             "upscale_ratio_bound", "upscale_levels"):
                setattr(stage, k, v[0] if len(v) else v)
        opt = stage
        keys_to_pass_to_nerf = ['triplane_channels', 'triplane_resolution', 'triplane_wavelet_levels', 'wavelet_type',
                                'hidden_dim', 'hidden_dim_color', 'hidden_dim_bg', 'learn_rotation_axis', 'dropout',
                                'inner_bound', 'lbound_auto_scale', 'upscale_ratio_bound', 'upscale_levels',
                                'density_blob_scale', 'density_blob_std', 'mlp_weight_decay', 'wavelet_base_resolution',
                                'nerfacc_renderer']
        extra = {{k: vars(opt)[k] for k in keys_to_pass_to_nerf}}
        model = NeRFNetwork(encoding="triplane_wavelet" if opt.triplane_wavelet else "hashgrid", bound=opt.bound,
                            cuda_ray=opt.cuda_ray, density_scale=opt.density_scale, min_near=opt.min_near,
                            density_thresh=opt.density_thresh, bg_radius=opt.bg_radius, **extra)
        C = opt.triplane_channels
        assert tuple(model.encoder.planes_features.shape) == (3, C, 64, 64)
        assert [tuple(p.shape) for p in model.encoder.planes_features_wavelet_coefs] == \\
            [(3, C, 3, 64 << i, 64 << i) for i in range(3)]
        assert model.encoder.output_dim == 3 * C and model.cascade == 2
        criterion = torch.nn.MSELoss(reduction='none')
        optimizer = lambda model: torch.optim.Adam(model.get_params(opt.lr), betas=(0.9, 0.99), eps=1e-15)
        scheduler = lambda optimizer: optim.lr_scheduler.LambdaLR(optimizer, lambda iter: decay_function(iter, opt))
        trainer = Trainer('trinerflet', opt, model, device=torch.device('cpu'), workspace=opt.workspace,
                          optimizer=optimizer, criterion=criterion, ema_decay=None, fp16=False, lr_scheduler=scheduler,
                          scheduler_update_every_step=True, metrics=[PSNRMeter()], use_checkpoint="scratch",
                          eval_interval=opt.save_every, mute=True, use_tensorboardX=False)
        n_opt = sum(p.numel() for g in trainer.optimizer.param_groups for p in g["params"])
        assert n_opt == sum(p.numel() for p in model.parameters() if p.requires_grad)
        # the reference's own checkpoint writer / loader around this model (utils.py:1390-1532)
        trainer.save_checkpoint(full=True)
        before = {{k: v.clone() for k, v in model.state_dict().items()}}
        with torch.no_grad():
            model.encoder.planes_features.add_(1.0)
        trainer.load_checkpoint()
        assert all(torch.equal(v, model.state_dict()[k]) for k, v in before.items())
        assert {{"encoder.planes_features", "encoder.planes_features_wavelet_coefs.0", "sigma_net.0.weight",
                "color_net.2.weight", "density_grid", "density_bitfield", "step_counter", "aabb_train"}} <= set(before)
        print("TRAINER_OK", n_opt)
    """)
    out = _run(body)
    assert "TRAINER_OK" in out


def test_reference_wrappers_bind_native_names_unchanged():
    """aux_libs/raymarching/raymarching.py:9-12 and aux_libs/shencoder/sphere_harmonics.py:9-12 do
    `import _raymarching as _backend` / `import _shencoder as _backend`; with install_backends() these are this
    build's modules, and every `_backend.<fn>(...)` call in the reference's wrapper files matches a function here
    in name and number of arguments (the prototypes of raymarching.h:7-17 / shencoder.h)."""
    out = _run(textwrap.dedent("""
        import importlib.util, inspect, re
        def load(name, path):
            spec = importlib.util.spec_from_file_location(name, path, submodule_search_locations=[os.path.dirname(path)])
            mod = importlib.util.module_from_spec(spec); sys.modules[name] = mod; spec.loader.exec_module(mod); return mod
        def header_arity(path):
            txt = open(path).read()
            return {m.group(1): len([a for a in m.group(2).split(",") if a.strip()])
                    for m in re.finditer(r"void\\s+(\\w+)\\s*\\(([^;]*)\\)\\s*;", txt)}
        for pkg, fname, native, hdr in (("raymarching", "raymarching.py", "_raymarching", "src/raymarching.h"),
                                        ("shencoder", "sphere_harmonics.py", "_shencoder", "src/shencoder.h")):
            base = f"/root/reference/aux_libs/{pkg}"
            mod = load(f"ref_{pkg}.{fname[:-3]}", f"{base}/{fname}")
            be = mod._backend
            assert be.__name__ == native and "/trinerflet_amd/backends/" in be.__file__, be
            used = set(re.findall(r"_backend\\.(\\w+)\\(", open(f"{base}/{fname}").read()))
            arity = header_arity(f"{base}/{hdr}")
            assert used <= set(arity), (used, arity)
            for fn, n in arity.items():
                assert len(inspect.signature(getattr(be, fn)).parameters) == n, (fn, n)
            print(native, sorted(arity))
        print("BACKENDS_OK")
    """))
    assert "BACKENDS_OK" in out
    assert "_raymarching ['composite_rays', 'composite_rays_train_backward', 'composite_rays_train_forward', " \
           "'march_rays', 'march_rays_train', 'morton3D', 'morton3D_invert', 'near_far_from_aabb', 'packbits', " \
           "'sph_from_ray']" in out


def test_ff_switch_constructs_the_reference_shapes_and_its_initial_weights(tmp_path):
    """`--ff` (main_nerf.py:31-34: `from nerf.network_ff import NeRFNetwork`, network_ff.py:7 `from ffmlp import FFMLP`).
    After install_dropin() both names resolve to this build.  Pinned against the reference's OWN aux_libs/ffmlp/ffmlp.py,
    imported here with its CUDA backend replaced by an empty stand-in (only `allocate_splitk` is touched at construction):
    the same parameter count, state-dict key, repr, and -- the initialisation is `manual_seed(42)` + uniform on the host --
    the same initial weights to the bit, for both networks of the `--ff` model."""
    out = _run(textwrap.dedent("""
        import importlib.util, torch
        import ffmlp, nerf.network_ff as nff
        assert "/trinerflet_amd/" in ffmlp.__file__ and "/trinerflet_amd/" in nff.__file__
        # the reference's module, backend stubbed
        be = types.ModuleType("_ffmlp"); be.allocate_splitk = lambda n: None; be.free_splitk = lambda: None
        sys.modules["_ffmlp"] = be
        tu = types.ModuleType("turtle"); tu.backward = tu.forward = None      # ffmlp.py:2 (a stray import; needs tkinter)
        sys.modules["turtle"] = tu
        spec = importlib.util.spec_from_file_location("ref_ffmlp", "/root/reference/aux_libs/ffmlp/ffmlp.py")
        ref = importlib.util.module_from_spec(spec); spec.loader.exec_module(ref)
        for args in ((48, 16, 64, 2), (32, 3, 64, 3), (144, 16, 128, 2), (32, 3, 128, 3)):
            a, b = ref.FFMLP(*args), ffmlp.FFMLP(*args)
            assert a.num_parameters == b.num_parameters and repr(a) == repr(b), (repr(a), repr(b))
            assert list(a.state_dict()) == list(b.state_dict()) == ["weights"]
            assert torch.equal(a.weights.detach(), b.weights.detach())
            assert (a.padded_output_dim, a.activation, a.output_activation) == (b.padded_output_dim, b.activation, b.output_activation)
        m = nff.NeRFNetwork(encoding="triplane_wavelet", bound=1.5, cuda_ray=True, density_scale=1, min_near=0.2,
                            density_thresh=10, bg_radius=-1, triplane_channels=16, triplane_resolution=64,
                            triplane_wavelet_levels=1, wavelet_type="bior6.8", hidden_dim=64, hidden_dim_color=64)
        keys = set(m.state_dict())
        assert {"sigma_net.weights", "color_net.weights", "encoder.planes_features", "density_grid", "density_bitfield"} <= keys
        assert m.in_dim == 48 and m.in_dim_color == 32 and len(m.get_params(1e-2)) == 4
        print("FF_OK")
    """))
    assert "FF_OK" in out
