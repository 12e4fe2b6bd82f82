"""GPU suite of the connected-components family (csrc/components.hip): every case of tests/components_cases.py under the three
neighbourhoods against tests/components_ref.py, element for element and with no renumbering; the tables, bit for bit; every
kernel-written buffer between guard bands; and the layers built on them (segmentation/components.py, routine.validate_lesions,
FCDMaskGenerator.lesion_report / clusters).  Everything is integer or a maximum, so every comparison is exact."""
import numpy as np
import pytest
import torch

from mri_epilepsy_diagnosis_amd import ops
from mri_epilepsy_diagnosis_amd.segmentation import components, routine

import components_cases as cc
import components_ref as ref
from guard import Guarded

pytestmark = pytest.mark.gpu

CASES = cc.build()
BY_NAME = {c.name: c for c in CASES}
_REF = {}


def _want(case, conn):
    """The reference labelling of a case, computed once and shared."""
    key = (case.name, conn)
    if key not in _REF:
        _REF[key] = ref.label(case.mask, conn, case.by_value)
    return _REF[key]


def _guarded(shape, dtype):
    """A kernel-written buffer of an integer or float dtype inside uint8 guard bands: (Guarded, the region viewed as dtype)."""
    esz = torch.empty((), dtype=dtype).element_size()
    g = Guarded(int(np.prod(shape, dtype=np.int64)) * esz, torch.uint8)
    return g, g.region.view(dtype).view(tuple(shape))


def _label_guarded(mask, conn, by_value=False):
    dev = torch.from_numpy(mask).cuda()
    g, out = _guarded(mask.shape, torch.int32)
    labels, count = ops.label_components(dev, conn, by_value, out=out)
    assert labels.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    g.assert_guards_intact("labels")
    assert not bool(g.untouched().view(-1, 4).all(1).any()), "a label was not written"
    return labels, count


@pytest.mark.parametrize("conn", cc.CONNECTIVITIES)
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_labels_equal_the_reference(case, conn):
    want, k = _want(case, conn)
    if case.expect is not None:
        assert k == case.expect[conn]
    labels, count = _label_guarded(case.mask, conn, case.by_value)
    assert count.dtype == torch.int32 and count.is_cuda and count.dim() == 0
    ref.assert_same_labelling(labels.cpu().numpy(), int(count), want, k, what="%s / %d" % (case.name, conn))


def test_scipy_aliases_and_bool_masks():
    case = BY_NAME["bernoulli_0.3_24x40x72"]
    dev = torch.from_numpy(case.mask).cuda()
    for alias, conn in ((1, 6), (2, 18), (3, 26)):
        a, ka = ops.label_components(dev, alias)
        b, kb = ops.label_components(dev.bool(), conn)
        assert torch.equal(a, b) and int(ka) == int(kb) == _want(case, conn)[1]
    assert int(ops.label_components(dev)[1]) == _want(case, 6)[1]                     # the default is scipy's: 6
    with pytest.raises(ValueError, match="connectivity"):
        ops.label_components(dev, 4)
    with pytest.raises(RuntimeError, match="uint8 or bool"):
        ops.label_components(dev.float())


@pytest.mark.parametrize("conn", cc.CONNECTIVITIES)
def test_two_runs_give_the_same_bits(conn):
    dev = torch.from_numpy(BY_NAME["bernoulli_0.6_tiles"].mask).cuda()
    a, ka = ops.label_components(dev, conn)
    b, kb = ops.label_components(dev, conn)
    assert torch.equal(a, b) and torch.equal(ka, kb)
    sa = ops.component_stats(a, int(ka), other=dev, score=dev.float())
    sb = ops.component_stats(b, int(kb), other=dev, score=dev.float())
    assert torch.equal(sa["stats"], sb["stats"]) and torch.equal(sa["peak"].view(torch.int32), sb["peak"].view(torch.int32))


def _stats_guarded(labels, capacity, rows, other=None, score=None, other_labels=None, other_capacity=None):
    """component_stats into guarded tables of `rows` >= capacity rows: (results, guards)."""
    gs, stats = _guarded((rows, 8), torch.int64)
    out, guards = {"stats": stats[:capacity]}, {"stats": gs}
    if score is not None:
        guards["peak"], peak = _guarded((rows,), torch.float32)
        out["peak"] = peak[:capacity]
    if other_labels is not None:
        guards["hit"], hit = _guarded((other_capacity,), torch.uint8)
        out["hit"] = hit
    res = ops.component_stats(labels, capacity, other=other, other_labels=other_labels, score=score, other_capacity=other_capacity,
                              out=out)
    torch.cuda.synchronize()
    for k, g in guards.items():
        assert res[k].data_ptr() == out[k].data_ptr()
        g.assert_guards_intact(k)
    return res, guards


@pytest.mark.parametrize("conn", cc.CONNECTIVITIES)
@pytest.mark.parametrize("name", ["bernoulli_0.3_tiles", "bernoulli_0.6_24x40x72", "snake", "class_map_by_value", "corners", "map_2d_9x70"])
def test_stats_peak_and_hit_equal_the_reference(name, conn):
    case = BY_NAME[name]
    want, k = _want(case, conn)
    rng = np.random.default_rng(7)
    other = (rng.random(case.mask.shape) < 0.35).astype(np.uint8) * rng.integers(1, 200, case.mask.shape).astype(np.uint8)
    score = rng.standard_normal(case.mask.shape).astype(np.float32)
    olab, ok = ref.label(other, conn)
    labels = torch.from_numpy(want).cuda()
    res, _ = _stats_guarded(labels, k, k, torch.from_numpy(other).cuda(), torch.from_numpy(score).cuda(), torch.from_numpy(olab).cuda(), ok)
    table, peak = ref.stats(want, k, other, score)
    got = {key: v.cpu().numpy() for key, v in res.items()}
    ref.assert_same_tables(got, {"stats": table, "peak": peak, "hit": ref.hit(want, olab, ok)}, what="%s / %d" % (name, conn))
    assert got["stats"][:, 0].sum() == (want > 0).sum() and (got["stats"][:, 0] > 0).all()
    # without the optional inputs: the overlap column is 0 and nothing else changes
    plain = ops.component_stats(labels, k)
    assert set(plain) == {"stats"}
    table0, _ = ref.stats(want, k)
    ref.assert_same_tables({"stats": plain["stats"].cpu().numpy()}, {"stats": table0})


def test_a_capacity_below_the_count_leaves_the_other_rows_alone():
    case = BY_NAME["bernoulli_0.3_tiles"]
    want, k = _want(case, 18)
    cap = k - 5
    assert cap > 3
    rng = np.random.default_rng(8)
    other = (rng.random(case.mask.shape) < 0.5).astype(np.uint8)
    score = rng.standard_normal(case.mask.shape).astype(np.float32)
    olab, ok = ref.label(other, 18)
    ocap = ok - 2
    assert ocap > 0
    res, guards = _stats_guarded(torch.from_numpy(want).cuda(), cap, k, torch.from_numpy(other).cuda(), torch.from_numpy(score).cuda(),
                                 torch.from_numpy(olab).cuda(), ocap)
    table, peak = ref.stats(want, cap, other, score)
    ref.assert_same_tables({key: v.cpu().numpy() for key, v in res.items()}, {"stats": table, "peak": peak, "hit": ref.hit(want, olab, ocap)})
    assert bool(guards["stats"].untouched()[cap * 64:].all()) and bool(guards["peak"].untouched()[cap * 4:].all())
    assert not bool(guards["stats"].untouched()[:cap * 64].view(-1, 8).all(1).any())
    # an empty row inside the capacity: the stated values
    few = ops.component_stats(torch.from_numpy(want).cuda(), k + 2, score=torch.from_numpy(score).cuda())
    d, h, w = want.shape
    assert few["stats"][k:].tolist() == [[0, 0, d, -1, h, -1, w, -1]] * 2 and few["peak"][k:].tolist() == [-np.inf] * 2


def test_select_components():
    case = BY_NAME["bernoulli_0.3_tiles"]
    want, k = _want(case, 6)
    labels = torch.from_numpy(want).cuda()
    rng = np.random.default_rng(9)
    keep = (rng.random(k + 1) < 0.5).astype(np.uint8)
    keep[0] = 0
    g, out = _guarded(want.shape, torch.uint8)
    got = ops.select_components(labels, torch.from_numpy(keep).cuda(), out=out)
    torch.cuda.synchronize()
    g.assert_guards_intact("selected mask")
    assert got.data_ptr() == out.data_ptr() and np.array_equal(got.cpu().numpy(), ref.select(want, keep))
    # a table shorter than the labels: ids beyond it select nothing; a bool table is taken as it is
    short = ops.select_components(labels, torch.from_numpy(keep[:k // 2].astype(bool)).cuda())
    assert np.array_equal(short.cpu().numpy(), ref.select(want, keep[:k // 2]))
    with pytest.raises(RuntimeError, match="int32"):
        ops.select_components(labels.long(), torch.from_numpy(keep).cuda())


def _lesion_volume():
    """Three ground-truth blobs and five predicted clusters in 20 x 24 x 40: blob A is hit by two clusters, blob B is missed, blob C
    is hit by one; two clusters are false alarms.  Cluster sizes hold a tie (the two 12-voxel clusters)."""
    gt = np.zeros((20, 24, 40), dtype=np.uint8)
    pred = np.zeros_like(gt)
    gt[2:8, 2:10, 2:12] = 1          # A
    gt[12:16, 3:7, 20:26] = 1        # B, missed
    gt[10:18, 14:22, 30:38] = 1      # C
    pred[3:5, 3:5, 1:4] = 1          # cluster on A: 12 voxels, 8 inside A
    pred[6:9, 8:12, 9:14] = 1        # second cluster on A: 60 voxels
    pred[11:17, 15:20, 31:36] = 1    # on C: 150 voxels
    pred[0:2, 18:20, 20:23] = 1      # false: 12 voxels (ties with the first)
    pred[18, 1, 1] = 1               # false: one voxel
    return pred, gt


@pytest.mark.parametrize("conn", (6, 26))
def test_lesion_scores_remove_small_keep_largest_rank_clusters(conn):
    pred, gt = _lesion_volume()
    dp, dg = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
    want = ref.lesion_scores(pred, gt, conn)
    assert (want["n_lesions"], want["n_clusters"], want["lesions_detected"], want["clusters_true"], want["clusters_false"]) == (3, 5, 2, 3, 2)
    assert want["sensitivity"] == 2 / 3 and want["precision"] == 3 / 5
    ref.assert_same_scores(components.lesion_scores(dp, dg, conn), want)
    ref.assert_same_scores(components.lesion_scores(dp.bool(), dg.bool(), conn), want)
    small = ref.lesion_scores(pred, gt, conn, min_voxels=12)
    assert small["n_clusters"] == 4 and small["clusters_false"] == 1
    ref.assert_same_scores(components.lesion_scores(dp, dg, conn, min_voxels=12), small)
    empty = components.lesion_scores(torch.zeros_like(dp), torch.zeros_like(dg), conn)
    ref.assert_same_scores(empty, ref.lesion_scores(np.zeros_like(pred), np.zeros_like(gt), conn))
    assert np.isnan(empty["sensitivity"]) and np.isnan(empty["precision"])
    ref.assert_same_scores(components.lesion_scores(dp, torch.zeros_like(dg), conn), ref.lesion_scores(pred, np.zeros_like(gt), conn))

    for n in (1, 12, 13, 61, 1000):
        got = components.remove_small(dp, n, conn)
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), ref.remove_small(pred, n, conn)), n
    for k in (0, 1, 2, 3, 4, 9):      # k = 3 cuts the tie: of the two 12-voxel clusters the one with the lower id (at z = 0) stays
        got = components.keep_largest(dp, k, conn)
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), ref.keep_largest(pred, k, conn)), k
    three = components.keep_largest(dp, 3, conn).cpu().numpy()
    assert three[0, 18, 20] == 1 and three[3, 3, 1] == 0

    rng = np.random.default_rng(10)
    score = rng.standard_normal(pred.shape).astype(np.float32)
    score[pred == 0] = 50.0                                       # the background's scores must not count
    score[3, 3, 1] = score[0, 18, 20] = 7.5                       # a tie of peaks: the lower id first
    for top_k in (None, 2, 4):
        got = components.rank_clusters(dp, torch.from_numpy(score).cuda(), conn, top_k)
        want_r = ref.rank_clusters(pred, score, conn, top_k)
        assert all(v.is_cuda for v in got.values())
        ref.assert_same_tables({k: v.cpu().numpy() for k, v in got.items()}, want_r)
    assert want_r["peaks"][0] == want_r["peaks"][1] == 7.5 and want_r["ids"][0] < want_r["ids"][1]


def test_components_object():
    pred, gt = _lesion_volume()
    c = components.components(torch.from_numpy(pred).cuda(), 26, other=torch.from_numpy(gt).cuda(), score=torch.from_numpy(pred).cuda().float())
    lab, k = ref.label(pred, 26)
    table, peak = ref.stats(lab, k, gt, pred.astype(np.float32))
    assert c.count == k and type(c.count) is int
    ref.assert_same_labelling(c.labels.cpu().numpy(), c.count, lab, k)
    ref.assert_same_tables({"sizes": c.sizes.cpu().numpy(), "boxes": c.boxes.cpu().numpy(), "overlap": c.overlap.cpu().numpy(),
                            "peak": c.peak.cpu().numpy(), "hit": c.hit.cpu().numpy()},
                           {"sizes": table[:, 0], "boxes": table[:, 2:], "overlap": table[:, 1], "peak": peak,
                            "hit": ref.hit(lab, *ref.label(gt, 26))})
    none = components.components(torch.zeros(4, 5, 6, dtype=torch.uint8, device="cuda"))
    assert none.count == 0 and none.sizes.numel() == 0 and tuple(none.boxes.shape) == (0, 6) and none.overlap is None and none.peak is None


def test_validate_lesions():
    from mri_epilepsy_diagnosis_amd.unet import UNet
    torch.manual_seed(1)
    model = UNet(in_channels=1, out_classes=2, dimensions=3, num_encoding_blocks=2, out_channels_first_layer=4, normalization="batch",
                 upsampling_type="linear", padding=True, activation="PReLU").cuda()
    with torch.no_grad():                        # an untrained classifier may call everything one class: balance it
        model.classifier.conv_layer.bias.zero_()
        w = model.classifier.conv_layer.weight
        w[1] = -w[0]
    loader = routine.synthetic_loader(2, 1, (16, 16, 16), "cuda", foreground=0.03)
    got = routine.validate_lesions(model, loader, connectivity=18, min_voxels=2)
    assert len(got) == 2
    model.eval()
    for i, batch in enumerate(loader):
        inputs, targets = routine.prepare_batch(batch, "cuda")
        with torch.no_grad():
            mask = ops.argmax_mask(routine.forward(model, inputs))[0].cpu().numpy()
        share = mask.mean()
        assert 0.02 < share < 0.98, "the mask is (nearly) one class: the scores below would pin nothing"
        want = ref.lesion_scores(mask, targets[0][0].cpu().numpy(), 18, 2)
        assert want["n_lesions"] > 1 and want["n_clusters"] > 0
        ref.assert_same_scores(got[i], want, what="volume %d" % i)
    default = routine.validate_lesions(model, loader)
    with torch.no_grad():
        mask = ops.argmax_mask(routine.forward(model, loader[0][routine.MRI][routine.DATA]))[0].cpu().numpy()
    ref.assert_same_scores(default[0], ref.lesion_scores(mask, loader[0][routine.LABEL][routine.DATA][0][0].cpu().numpy(), 26, 0))


def test_fcd_mask_generator_lesion_report_and_clusters():
    from mri_epilepsy_diagnosis_amd.detection.mask import FCDMaskGenerator
    from mri_epilepsy_diagnosis_amd.detection.model import PatchModel
    x, y, z, h, w = 40, 24, 5, 4, 4
    gm = torch.zeros(x, y, z, device="cuda")
    gm[3:37] = 1.0                               # six whole strips of four rows per slice; the template starts in column 3
    gen = FCDMaskGenerator(PatchModel(), gm, h, w)
    r = gen.plan.strips
    rng = np.random.default_rng(11)
    patch_map = torch.from_numpy((rng.random((4, r, z)) < 0.4).astype(np.uint8)).cuda()
    pred = gen.masking(patch_map)                                             # a painted mask
    assert 0 < int(pred.sum()) < pred.numel()
    true = torch.from_numpy((rng.random((x, y, z)) < 0.02).astype(np.float32) * 3.0).cuda()
    for conn in (6, 26):
        want = ref.lesion_scores(pred.cpu().numpy(), true.cpu().numpy() > 0, conn)
        ref.assert_same_scores(gen.lesion_report(pred, true, conn), want)
    assert want["n_clusters"] > 0 and want["n_lesions"] > 1
    with pytest.raises(RuntimeError, match="wrong shape"):
        gen.lesion_report(pred, true[1:])
    lab, k = ref.label(pred.cpu().numpy(), 26)
    table, _ = ref.stats(lab, k)
    order = np.array(sorted(range(k), key=lambda i: (-table[i, 0], i)), dtype=np.int64)
    for top_k in (None, 1):
        got = gen.clusters(pred, top_k)
        o = order if top_k is None else order[:top_k]
        ref.assert_same_tables({key: v.cpu().numpy() for key, v in got.items()}, {"ids": o + 1, "sizes": table[o, 0], "boxes": table[o][:, 2:]})
