"""GPU: the FID feature extractor (freefine_amd/inception.py HipFIDInception) against tests/inception_ref.py in fp64, and the drivers on top of it.

The gate is the single-precision yardstick: the restatement is run in fp32 on the CPU in the same test, its deviation from the fp64 run is the size of error
fp32 arithmetic makes on this network and these inputs, and the device may deviate by inception_ref.MARGIN = 4 times that (only the order of the sums
differs) -- both relative to the scale of the compared map.  Measured values are printed before they are asserted on."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import inception_ref as IR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}


def setup(config, side, batch):
    """(state fp64, uint8 images [batch, 224, 224, 3], the four block outputs of the restatement in fp64 and in fp32), computed once per configuration"""
    key = (config, side, batch)
    if key not in _CACHE:
        st = IR.seeded_state(IR.network_shapes(config), 100 + side)
        img = torch.randint(0, 256, (batch, 224, 224, 3), generator=torch.Generator().manual_seed(side), dtype=torch.uint8)
        img[:, :112] = (img[:, :112].float() * 0.4).to(torch.uint8)          # some structure: not every image has the same statistics
        with torch.no_grad():
            b64 = IR.forward(st, IR.prepare(img, torch.float64), side)
            b32 = IR.forward({k: v.float() for k, v in st.items()}, IR.prepare(img, torch.float32), side)
        _CACHE[key] = (st, img, b64, b32)
    return _CACHE[key]


def deviation(a, ref):
    return ((a.double() - ref).abs().max() / ref.abs().max()).item()


def gate(what, got, r64, r32):
    e_dev, e_ref = deviation(got, r64), deviation(r32, r64)
    print(f"{what}: device vs fp64 {e_dev:.3e}, torch fp32 vs fp64 {e_ref:.3e} of the scale {r64.abs().max().item():.3f}; gate {IR.MARGIN * e_ref:.3e}")
    assert torch.isfinite(got).all() and e_ref > 0 and e_dev <= IR.MARGIN * e_ref, (what, e_dev, e_ref)


@pytest.mark.parametrize("config,side,batch", [("tiny", 75, 3), ("tiny", 107, 3), ("full", 299, 2)])
def test_features_against_the_fp64_restatement(gpu, config, side, batch):
    from freefine_amd.inception import HipFIDInception
    st, img, b64, b32 = setup(config, side, batch)
    net = HipFIDInception(config, st, device=gpu, side=side)
    f = net.features_224(img.to(gpu)).cpu()
    assert f.shape == (batch, 2048 if config == "full" else 256) and f.dtype == torch.float32 and net.dim == f.shape[1]
    gate(f"{config} at {side}, batch {batch}: pool3 features", f, b64[3].flatten(1), b32[3].flatten(1))
    again = net.features_224(img.to(gpu)).cpu()
    assert torch.equal(f.view(torch.int32), again.view(torch.int32))
    one = net.features_224(img[1:2].to(gpu)).cpu()                          # a row does not depend on its batch
    assert torch.equal(one.view(torch.int32), f[1:2].view(torch.int32))


@pytest.mark.parametrize("side", [75, 107])
def test_block_boundaries_name_a_wrong_layer(gpu, side):
    """the outputs of pytorch-fid's four blocks in the tiny configuration: the 64-, 192-, 768- and 2048-channel maps of the full network (8, 24, 96, 256 here)"""
    from freefine_amd.inception import HipFIDInception
    st, img, b64, b32 = setup("tiny", side, 3)
    net = HipFIDInception("tiny", st, device=gpu, side=side)
    got = net.features_224(img.to(gpu), blocks=True)
    assert [g.shape[3] for g in got] == [8, 24, 96, 256]
    for i, (g, r64, r32) in enumerate(zip(got, b64, b32)):
        g = g.cpu().permute(0, 3, 1, 2)
        assert g.shape == r64.shape, (i, g.shape, r64.shape)
        gate(f"tiny at {side}: block {i} {tuple(r64.shape)}", g, r64, r32)


def write_images(tmp_path):
    """eight PNGs of three non-square sizes, interleaved: with batch_size 3 the five of one size span a batch boundary"""
    from PIL import Image
    rng = np.random.default_rng(8)
    sizes = [(40, 56), (64, 48), (40, 56), (90, 33), (40, 56), (64, 48), (40, 56), (40, 56)]
    files = []
    for i, (h, w) in enumerate(sizes):
        im = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        im[:h // 2] = (im[:h // 2] * rng.uniform(0.1, 1.0)).astype(np.uint8)
        files.append(str(tmp_path / f"im{i}.png"))
        Image.fromarray(im).save(files[-1])
    return files


def test_activations_of_files_keep_their_order_across_batches(gpu, tmp_path):
    from PIL import Image
    from freefine_amd import metrics as FM
    from freefine_amd.inception import HipFIDInception
    st = setup("tiny", 75, 3)[0]
    net = HipFIDInception("tiny", st, device=gpu, side=75)
    files = write_images(tmp_path)
    got = FM.get_inception_activations(files, net, batch_size=3)
    assert got.dtype == np.float64 and got.shape == (8, 256)
    small = torch.from_numpy(np.stack([IR.pil_resize(np.asarray(Image.open(f).convert("RGB"))) for f in files]))
    with torch.no_grad():
        r64, r32 = IR.features(st, small, 75), IR.features(st, small, 75, torch.float32)
    gate("get_inception_activations on 8 files, batch_size 3", torch.from_numpy(got), r64, r32)
    d = (torch.from_numpy(got)[:, None] - r64[None]).abs().amax(2)          # row i is nearest to reference row i: the order is the files'
    assert d.argmin(1).tolist() == list(range(8))
    alone = FM.get_inception_activations(files[4:5], net)
    assert np.array_equal(alone[0], got[4])


def test_drivers_and_the_command_line(gpu, tmp_path):
    from freefine_amd import metrics as FM
    from freefine_amd.inception import HipFIDInception
    st = {k: v.float() for k, v in setup("tiny", 75, 3)[0].items()}          # as a checkpoint file holds it
    net = HipFIDInception("tiny", st, device=gpu, side=75)
    real_root = tmp_path / "real"
    real_root.mkdir()
    real = write_images(real_root)
    (tmp_path / "gen").mkdir()
    gen = write_images(tmp_path / "gen")[:6]
    data = {"a": {"instances": {"0": {f"c{i}": {"ori_img_path": "unused", "gen_img_path": g} for i, g in enumerate(gen)}}}}
    value = FM.calculate_fid(data, "gen_img_path", str(real_root), net, batch_size=3)
    r, g = FM.parse_data(data, "gen_img_path", str(real_root))
    assert sorted(r) == sorted(real) and g == gen
    fr, fg = FM.get_inception_activations(r, net, 3), FM.get_inception_activations(g, net, 3)
    want = FM.frechet_distance(fr.mean(0), np.cov(fr, rowvar=False), fg.mean(0), np.cov(fg, rowvar=False))
    print(f"calculate_fid over 8 real and 6 generated files (tiny): {value}")
    assert isinstance(value, float) and np.isfinite(value) and value == want
    from_state = FM.calculate_fid(data, "gen_img_path", str(real_root), st, batch_size=3, config="tiny", side=75)
    assert from_state == value
    weights, jpath = str(tmp_path / "inception_tiny.pth"), str(tmp_path / "results.json")
    torch.save(st, weights)
    json.dump(data, open(jpath, "w"))
    main = os.path.join(ROOT, "evaluation", "metrics", "main.py")
    run = subprocess.run([sys.executable, main, "--path", jpath, "--task", "100000000", "--fid_weights", weights, "--fid_path", str(real_root), "--fid_config", "tiny"],
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout, run.stderr)
    line = [ln for ln in run.stdout.splitlines() if ln.startswith("FID: ")]
    assert len(line) == 1 and float(line[0][5:]) == value, run.stdout
