"""bench.py's bookkeeping that needs no GPU: which kernels a section's counter traffic is summed over."""
import csv
import glob
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _short(name):
    m = re.search(r"(k_[a-z0-9_]+)", name)
    return m.group(1) if m else name


def test_every_profiled_kernel_of_a_section_is_owned_by_it():
    """Round 5's line carried top[2].traffic_over_algorithmic = 0.014: the field backward's traffic was summed over
    k_slab_reduce alone because "k_field_bwd_rows" was matched by equality against "k_field_bwd".  The kernel names of the
    committed rocprof statistics (a real base run) are the fixture: every one of them lands in the section it belongs to,
    and in no other."""
    import bench
    names = set()
    for f in glob.glob(os.path.join(ROOT, "profiles", "r0[56]*_bench_base_kernel_stats.csv")):
        with open(f) as fh:
            names |= {_short(r["Name"]) for r in csv.DictReader(fh) if "k_" in r["Name"]}
    assert {"k_field_bwd_rows", "k_idwt_bwd_walk", "k_to_texel_major_h", "k_adam_l1_live"} <= names
    want = {"k_field_bwd_rows": "field_bwd", "k_slab_reduce": "field_bwd", "k_field_fwd": "field_fwd",
            "k_idwt_bwd_walk": "idwt_adjoint", "k_idwt_bwd_pipe": "idwt_adjoint", "k_idwt_fwd_walk": "idwt_fwd",
            "k_idwt_fwd_pipe": "idwt_fwd", "k_to_texel_major_h": "idwt_fwd", "k_tile_accumulate": "plane_grad_binned",
            "k_adam_l1_live": "adam_coef", "k_adam_l1": "adam_coef", "k_adam_record": "adam_coef"}
    for kn in names:
        owners = [s for s in bench.SECTION_KERNELS if bench.section_owns(s, kn)]
        assert owners == ([want[kn]] if kn in want else []), (kn, owners)
    # the replay of the deferred pass is not part of the per-step coefficient pass
    assert not bench.section_owns("adam_coef", "k_adam_l1_catchup")
    # hidden 128's two-launch backward (templated name, csrc/field_bwd.hip) belongs to the same section
    assert bench.section_owns("field_bwd", _short("void (anonymous namespace)::k_field_bwd<48, 128, 1>(Args)"))


def test_dump_outputs_writes_the_same_sample_every_time(tmp_path):
    """bench.dump_outputs (--dump-outputs): float32 .npy per output, arrays above DUMP_SAMPLE elements as the values at
    fixed seeded positions -- the same positions in every run, so two builds compare file for file."""
    import numpy as np
    import torch
    import bench
    from trinerflet_amd import synthetic
    from trinerflet_amd.nerf.network import NeRFNetwork

    class _Step:
        pass

    def model():
        m = NeRFNetwork(encoding="triplane_wavelet", bound=1.5, cuda_ray=True, density_thresh=10, hidden_dim=64,
                        hidden_dim_color=64, triplane_channels=16, triplane_resolution=256, triplane_wavelet_levels=4,
                        wavelet_type="bior6.8")
        synthetic.init_field_parameters(m, seed=0)
        return m

    ts = _Step()
    rng = np.random.default_rng(0)
    ts.last = {"mse": torch.tensor(0.25), "wavelet_reg": torch.tensor(0.5), "image": torch.from_numpy(rng.random((64, 3))),
               "ws": torch.from_numpy(rng.random(64)), "depth": torch.from_numpy(rng.random(64)), "M": 7}
    dumps = []
    for k in range(2):
        m = model()
        out = tmp_path / f"d{k}"
        nbytes = bench.dump_outputs(str(out), torch.tensor(0.75), m, ts)
        files = {f.name[:-4]: np.load(f) for f in out.iterdir()}
        assert nbytes == sum(a.nbytes for a in files.values()) <= bench.DUMP_BUDGET
        assert all(a.dtype == np.float32 for a in files.values())
        dumps.append(files)
    a, b = dumps
    assert set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)
    assert float(a["loss"]) == 0.75 and a["image"].shape == (64, 3) and "M" not in a
    assert {"param." + n for n, _ in m.named_parameters()} | {"buffer.density_grid"} <= set(a)
    assert a["param.encoder.planes_features"].shape == (3, 16, 64, 64)       # small: whole
    big = "param.encoder.planes_features_wavelet_coefs.1"                     # 3 x 16 x 3 x 128^2: sampled
    full = dict(m.named_parameters())[big[len("param."):]].detach().reshape(-1).numpy()
    assert full.size > bench.DUMP_SAMPLE and a[big].shape == (bench.DUMP_SAMPLE,)
    import zlib
    idx = np.sort(np.random.default_rng(zlib.crc32(big.encode())).integers(0, full.size, bench.DUMP_SAMPLE))
    assert np.array_equal(a[big], full[idx])


def test_sections_is_refused_without_full():
    """--sections prints the instrumented pass after the timed steps, which only --full runs: without --full the
    arguments are refused before anything touches a GPU."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--sections"], capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode == 2 and "--full" in r.stderr, r.stderr[-1000:]
