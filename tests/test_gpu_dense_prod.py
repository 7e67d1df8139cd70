"""lfd_dense_prod_kernel - the ordered dense kernel instantiated for the production shape (csrc/lfd_kernels.hip) - writes the
bytes of the generic lfd_dense_kernel, and lfd_triangulate_dense launches it only where lfd_dense_variant says it may.  The shapes are the
smallest at which the instantiation can go wrong: one tile per reference with every wave on half a grid row and a look-back across the
reference boundary, two tiles per reference, a tile that spans two grid rows, one and four neighbours.  ``pytest -m gpu``."""
import numpy as np
import pytest
import torch

import lichtfeld_densification_plugin_amd as lfd
from lichtfeld_densification_plugin_amd import synthetic
from lichtfeld_densification_plugin_amd.core import hip_backend as hb

pytestmark = pytest.mark.gpu

WM = HM = 512
REFS = (0, 60)
# name: (k, H, W)
SHAPES = {"one_tile_per_ref": (3, 4, 256), "two_tiles_per_ref": (3, 8, 256), "tile_spans_two_rows": (3, 4, 512), "k1": (1, 4, 256), "k4": (4, 8, 256)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cams():
    return synthetic.ring_cameras(185, width=1297, height=840, focal=960.0, seed=0)


@pytest.fixture(scope="module")
def dens(dev, cams):
    d = hb.HipDensifier(dev)
    d.upload_cameras(cams)
    yield d
    d.close()


_scenes = {}


def scene(cams, dev, k, H, W, channels=2):
    """The references of a shape (made once): 0.5 px of matching noise and the generator's 5 % gross outliers."""
    key = (k, H, W, channels)
    if key not in _scenes:
        refs = []
        for ref in REFS:
            nbrs = synthetic.ring_neighbours(len(cams), ref, k)
            s = synthetic.synth_reference(cams, ref, nbrs, H, W, WM, HM, noise_px=0.5, outlier_frac=0.05, channels=channels, seed=1000 + ref, cert_mode="smooth")
            refs.append(hb.ReferenceInputs(ref_cam=ref, nbr_cams=nbrs, cert=[s.cert[j].to(dev) for j in range(k)],
                                           warp=[s.warp[j].contiguous().to(dev) for j in range(k)], image=s.image.to(dev)))
        _scenes[key] = refs
    return _scenes[key]


def config(k, **kw):
    kw.setdefault("reproj_thresh", 0.8)
    return lfd.DensePipelineConfig(output_path="", nns_per_ref=k, **kw)


def launch(dens, batch, params, with_cell=False, with_segments=False, generic=None, monkeypatch=None):
    """One lfd_triangulate_dense into fresh buffers -> (variant the predicate names, buffers, ref_offsets).  ``generic``: with LFD_DENSE_GENERIC=1."""
    if generic:
        monkeypatch.setenv("LFD_DENSE_GENERIC", "1")
        dens.reload_env()
    try:
        out = hb.OutputBuffers(batch.n_refs * batch.H * batch.W, batch.n_refs, batch.k, dens.device, with_cell=with_cell, with_segments=with_segments)
        variant = hb.dense_variant(batch.c, params, out.c, out.seg_counts.data_ptr() if with_segments else None)
        dens.launch_dense(batch, params, out)
        dens.check_launches()
        return variant, out, out.ref_offsets.cpu().numpy().copy()
    finally:
        if generic:
            monkeypatch.delenv("LFD_DENSE_GENERIC")
            dens.reload_env()


def same_bytes(a, b, n):
    return torch.equal(a[:n].contiguous().view(torch.int32), b[:n].contiguous().view(torch.int32))


@pytest.mark.parametrize("name", list(SHAPES))
def test_production_kernel_writes_the_generic_kernels_bytes(dev, cams, dens, monkeypatch, name):
    k, H, W = SHAPES[name]
    batch = hb.PreparedBatch(scene(cams, dev, k, H, W), WM, HM, cameras=cams)
    params = hb.make_params(config(k))
    v_prod, prod, offs_prod = launch(dens, batch, params)
    assert v_prod == 1, "the predicate does not name the production kernel for this shape"
    v_gen, gen, offs_gen = launch(dens, batch, params, generic=True, monkeypatch=monkeypatch)
    n = int(offs_gen[-1])
    cells = len(REFS) * H * W
    print(name, "survivors", n, "of", cells, "per reference", np.diff(offs_gen))
    assert 0 < n < cells                                  # neither an empty nor an all-kept cloud
    assert (np.diff(offs_gen) > 0).all()                  # ... in either reference: the look-back crosses the boundary with a count
    np.testing.assert_array_equal(offs_prod, offs_gen)
    assert same_bytes(prod.xyz, gen.xyz, n) and same_bytes(prod.rgb, gen.rgb, n) and same_bytes(prod.err, gen.err, n)
    # launches back to back on one context (tickets and look-back epochs move on): the same bytes again
    for _ in range(2):
        _, again, offs_again = launch(dens, batch, params)
        np.testing.assert_array_equal(offs_again, offs_gen)
        assert same_bytes(again.xyz, gen.xyz, n) and same_bytes(again.rgb, gen.rgb, n) and same_bytes(again.err, gen.err, n)


def test_the_comparison_input_fails_both_gates(dev, cams, dens, monkeypatch):
    """The generic kernel's own counts on the compared input: some cells fail the Sampson gate and some fail the reprojection test.  Each count
    is what the generic kernel keeps with neither test (and no parallax test: cheirality alone) minus what it keeps with that ONE test added.
    (On this input every cell the Sampson gate rejects fails the reprojection test as well - the CPU twin says so - hence one test at a time.)"""
    k, H, W = SHAPES["two_tiles_per_ref"]
    batch = hb.PreparedBatch(scene(cams, dev, k, H, W), WM, HM, cameras=cams)
    count = lambda **kw: int(launch(dens, batch, hb.make_params(config(k, min_parallax_deg=0.0, **kw)), generic=True, monkeypatch=monkeypatch)[2][-1])
    neither = count(sampson_thresh=0.0, reproj_thresh=1e6)
    failed_sampson = neither - count(reproj_thresh=1e6)
    failed_reproj = neither - count(sampson_thresh=0.0)
    print("cells past cheirality", neither, "of them failing Sampson", failed_sampson, "failing reprojection", failed_reproj)
    assert failed_sampson > 0 and failed_reproj > 0


def _masked(refs, dev):
    m = torch.ones((HM, WM), dtype=torch.uint8, device=dev)
    m[:, :WM // 3] = 0
    return [hb.ReferenceInputs(ref_cam=r.ref_cam, nbr_cams=r.nbr_cams, cert=r.cert, warp=r.warp, image=r.image, mask_a=m if i == 0 else None)
            for i, r in enumerate(refs)]


# one launch per row of the table the production kernel assumes: what differs from the compared launch
VIOLATIONS = {
    "grid_6x256": dict(grid=(6, 256)),
    "mask": dict(mask=True),
    "warp_channels_4": dict(channels=4),
    "explicit_axes": dict(axes=True),
    "certainty_thresh_0": dict(cfg=dict(certainty_thresh=0.0)),
    "no_filter": dict(cfg=dict(no_filter=True)),
    "sampson_thresh_0": dict(cfg=dict(sampson_thresh=0.0)),
    "min_parallax_deg_0": dict(cfg=dict(min_parallax_deg=0.0)),
    "with_cell": dict(with_cell=True),
    "with_segments": dict(with_segments=True),
    "exact_colour": dict(exact=True),
}


@pytest.mark.parametrize("name", list(VIOLATIONS))
def test_a_violated_assumption_launches_the_generic_kernel(dev, cams, dens, name):
    v = VIOLATIONS[name]
    k = 3
    H, W = v.get("grid", (8, 256))
    refs = scene(cams, dev, k, H, W, channels=v.get("channels", 2))
    if v.get("mask"):
        refs = _masked(refs, dev)
    axes = [synthetic.identity_axis_torch(W, dev), synthetic.identity_axis_torch(H, dev)] if v.get("axes") else None
    batch = hb.PreparedBatch(refs, WM, HM, axes=axes, cameras=cams)
    params = hb.make_params(config(k, **v.get("cfg", {})), exact_colour=bool(v.get("exact")))
    variant, out, offs = launch(dens, batch, params, with_cell=bool(v.get("with_cell")), with_segments=bool(v.get("with_segments")))
    assert variant == 0
    n = int(offs[-1])
    assert 0 < n <= len(REFS) * H * W and (np.diff(offs) >= 0).all()
    assert bool(torch.isfinite(out.xyz[:n]).all())
    if v.get("with_segments"):
        assert int(out.seg_counts.sum()) == n
    if v.get("with_cell"):
        assert int(out.cell[:n].max()) < H * W and int(out.slot[:n].max()) < k
