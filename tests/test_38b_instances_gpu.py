"""GPU: query.segment_instances and query.component_filter (one knn.neighbors and one knn.components call each) against the
restatement composed in NumPy, on the planted scenes of tests/knn_components_cases.py -- whose geometry
tests/test_knn_components_host.py checks on the CPU."""
import numpy as np
import pytest
import torch

from tests import knn_components_cases as cc
from tests import knn_components_restatement as cr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def instance_scene(gpu_device):
    from opengaussian_amd import knn
    pts, lab, blob = cc.instance_scene()
    xyz = torch.from_numpy(pts).to(gpu_device)
    idx, d2 = knn.neighbors(xyz, cc.INSTANCE_K)
    return dict(pts=pts, lab=lab, blob=blob, xyz=xyz, labels=torch.from_numpy(lab).to(gpu_device), table=(idx, d2),
                idx=idx.cpu().numpy(), d2=d2.cpu().numpy())


def _equal(got, want):
    assert isinstance(got[1], int) and got[1] == want[1]
    assert got[0].dtype is torch.int32 and np.array_equal(got[0].cpu().numpy(), want[0])
    assert np.array_equal(got[2].cpu().numpy(), want[2]) and np.array_equal(got[3].cpu().numpy(), want[3])


@pytest.mark.parametrize("min_size,ignore", [(1, None), (cc.FLOATER + 1, None), (cc.FLOATER + 1, (7,)), (1, (7, 0))])
def test_segment_instances_equals_the_restatement(instance_scene, min_size, ignore):
    from opengaussian_amd import query
    s = instance_scene
    want = cr.segment_instances(s["idx"], s["d2"], s["lab"], cc.INSTANCE_MAX_DIST, min_size, ignore or ())
    _equal(query.segment_instances(s["xyz"], s["labels"], k=cc.INSTANCE_K, max_dist=cc.INSTANCE_MAX_DIST, min_size=min_size,
                                   ignore=ignore), want)
    _equal(query.segment_instances(s["xyz"], s["labels"], max_dist=cc.INSTANCE_MAX_DIST, min_size=min_size, ignore=ignore,
                                   neighbors=s["table"]), want)


def test_segment_instances_finds_the_blobs_and_drops_the_floaters(instance_scene):
    from opengaussian_amd import query
    s = instance_scene
    lab, blob = s["lab"], s["blob"]
    inst, num, ilab, isize = query.segment_instances(s["xyz"], s["labels"], k=cc.INSTANCE_K, max_dist=cc.INSTANCE_MAX_DIST,
                                                     min_size=cc.FLOATER + 1, ignore=(7,))
    inst, ilab, isize = inst.cpu().numpy(), ilab.cpu().numpy(), isize.cpu().numpy()
    counted = [b for b in range(blob.max() + 1) if lab[blob == b][0] != 7]
    assert num == len(counted)
    for b in counted:
        ids = np.unique(inst[blob == b])
        assert len(ids) == 1 and ids[0] >= 0 and isize[ids[0]] == (blob == b).sum() and ilab[ids[0]] == lab[blob == b][0]
    floaters = (blob == -1) & (lab >= 0)
    assert (inst[floaters] == -1).all() and (inst[lab == 7] == -1).all() and (inst[lab == -1] == -1).all()
    kept, num1, _, size1 = query.segment_instances(s["xyz"], s["labels"], k=cc.INSTANCE_K, max_dist=cc.INSTANCE_MAX_DIST, ignore=(7,))
    assert num1 == num + 2 and bool((kept.cpu().numpy()[floaters] >= 0).all()) and sorted(size1.tolist())[:2] == [cc.FLOATER] * 2
    rows = torch.from_numpy(lab == 7).to(s["xyz"].device)                   # a bool ignore marks rows
    _equal(query.segment_instances(s["xyz"], s["labels"], max_dist=cc.INSTANCE_MAX_DIST, ignore=rows, neighbors=s["table"]),
           cr.segment_instances(s["idx"], s["d2"], lab, cc.INSTANCE_MAX_DIST, 1, (7,)))
    none = query.segment_instances(s["xyz"], torch.full_like(s["labels"], -1), neighbors=s["table"])
    assert none[1] == 0 and bool((none[0] == -1).all()) and none[2].numel() == 0 and none[3].numel() == 0


def test_component_filter_keeps_the_main_blobs_and_drops_what_outlier_mask_keeps(gpu_device):
    from opengaussian_amd import knn, query
    pts, grp, main = cc.filter_scene()
    xyz, group = torch.from_numpy(pts).to(gpu_device), torch.from_numpy(grp).to(gpu_device)
    G = cc.FILTER_GROUPS
    floater = ~main & (grp >= 0) & (grp < G)
    keep = query.component_filter(xyz, group, G, k=cc.FILTER_K)
    assert keep.dtype is torch.bool and np.array_equal(keep.cpu().numpy(), main)               # exactly the planted main blobs
    assert knn.outlier_mask(xyz, group, G).cpu().numpy()[floater].all()                         # the dense floater passes that one
    idx, d2 = knn.neighbors(xyz, cc.FILTER_K)
    idx, d2 = idx.cpu().numpy(), d2.cpu().numpy()
    for share, max_dist in ((None, 0.05), (None, 0.3), (0.0, None), (0.05, None), (40 / 340, None), (0.5, None), (1.0, None), (0.1, 0.05)):
        want = cr.component_filter(idx, d2, grp, G, max_dist, share)
        got = query.component_filter(xyz, group, G, k=cc.FILTER_K, max_dist=max_dist, min_share=share)
        assert np.array_equal(got.cpu().numpy(), want), (share, max_dist)
    one = query.component_filter(xyz, k=cc.FILTER_K)
    assert np.array_equal(one.cpu().numpy(), cr.component_filter(idx, d2, None, 1))
    assert query.component_filter(torch.zeros((0, 3), device=gpu_device), k=4).shape == (0,)


def test_status_word_is_clean_after_the_module(gpu_device):
    from opengaussian_amd import _lib
    torch.cuda.synchronize()
    assert _lib.lib().ogs_check_async_status() == 0
