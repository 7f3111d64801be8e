"""GPU: query.segment_instances_dbscan and query.density_filter (one knn.dbscan call each) against the restatement composed in
NumPy, on the planted scenes of tests/knn_components_cases.py and tests/knn_radius_cases.py -- whose geometry
tests/test_knn_radius_host.py checks on the CPU."""
import numpy as np
import pytest
import torch

from tests import knn_components_cases as cc
from tests import knn_radius_cases as rc
from tests import knn_radius_restatement as rr

pytestmark = pytest.mark.gpu


def _equal(got, want):
    assert isinstance(got[1], int) and got[1] == want[1]
    assert got[0].dtype is torch.int32 and np.array_equal(got[0].cpu().numpy(), want[0])
    assert np.array_equal(got[2].cpu().numpy(), want[2]) and np.array_equal(got[3].cpu().numpy(), want[3])


@pytest.mark.parametrize("min_size,ignore", [(1, None), (cc.FLOATER + 1, None), (20, (7,)), (1, (7, 0))])
def test_segment_instances_dbscan_equals_the_restatement(gpu_device, min_size, ignore):
    from opengaussian_amd import query
    pts, lab, blob = cc.instance_scene()
    xyz, labels = torch.from_numpy(pts).to(gpu_device), torch.from_numpy(lab).to(gpu_device)
    want = rr.segment_instances_dbscan(pts, lab, rc.INSTANCE_EPS, rc.INSTANCE_MIN_PTS, min_size, ignore or ())
    got = query.segment_instances_dbscan(xyz, labels, rc.INSTANCE_EPS, rc.INSTANCE_MIN_PTS, min_size=min_size, ignore=ignore)
    _equal(got, want)
    assert got[1] >= 4 and got[2].dtype is labels.dtype
    if ignore == (7,):
        rows = torch.from_numpy(lab == 7).to(gpu_device)                    # a bool ignore marks rows
        _equal(query.segment_instances_dbscan(xyz, labels, rc.INSTANCE_EPS, rc.INSTANCE_MIN_PTS, min_size=min_size, ignore=rows), want)


def test_a_thin_bridge_keeps_two_instances_where_the_knn_graph_merges_them(gpu_device):
    from opengaussian_amd import query
    pts, lab, part = rc.bridge_scene()
    xyz, labels = torch.from_numpy(pts).to(gpu_device), torch.from_numpy(lab).to(gpu_device)
    inst, num, ilab, isize = query.segment_instances_dbscan(xyz, labels, rc.BRIDGE_EPS, rc.BRIDGE_MIN_PTS)
    _equal((inst, num, ilab, isize), rr.segment_instances_dbscan(pts, lab, rc.BRIDGE_EPS, rc.BRIDGE_MIN_PTS))
    inst = inst.cpu().numpy()
    a, b = np.unique(inst[part == 0]), np.unique(inst[part == 1])
    assert num == 2 and len(a) == 1 and len(b) == 1 and a[0] >= 0 and b[0] >= 0 and a[0] != b[0]
    merged, one, _, size = query.segment_instances(xyz, labels, k=rc.BRIDGE_K, max_dist=rc.BRIDGE_EPS)
    assert one == 1 and not merged.any() and size.tolist() == [len(pts)]    # the kNN graph under the same distance joins them
    none = query.segment_instances_dbscan(xyz, torch.full_like(labels, -1), rc.BRIDGE_EPS)
    assert none[1] == 0 and bool((none[0] == -1).all()) and none[2].numel() == 0 and none[3].numel() == 0


def test_density_filter_keeps_the_main_blobs(gpu_device):
    from opengaussian_amd import query
    pts, grp, main = cc.filter_scene()
    xyz, group = torch.from_numpy(pts).to(gpu_device), torch.from_numpy(grp).to(gpu_device)
    G = cc.FILTER_GROUPS
    for share in (None, 0.5, 0.2):
        keep = query.density_filter(xyz, group, G, eps=rc.FILTER_EPS, min_pts=rc.FILTER_MIN_PTS, min_share=share)
        assert keep.dtype is torch.bool and np.array_equal(keep.cpu().numpy(), main), share           # exactly the planted main blobs
    for share, eps in ((0.05, rc.FILTER_EPS), (None, 0.05), (0.0, 0.05), (1.0, rc.FILTER_EPS)):
        want = rr.density_filter(pts, grp, G, eps, rc.FILTER_MIN_PTS, share)
        got = query.density_filter(xyz, group, G, eps=eps, min_pts=rc.FILTER_MIN_PTS, min_share=share)
        assert np.array_equal(got.cpu().numpy(), want), (share, eps)
    one = query.density_filter(xyz, eps=rc.FILTER_EPS)
    assert np.array_equal(one.cpu().numpy(), rr.density_filter(pts, None, 1, rc.FILTER_EPS))
    assert query.density_filter(torch.zeros((0, 3), device=gpu_device), eps=0.1).shape == (0,)
    with pytest.raises(ValueError):
        query.density_filter(xyz, group, G)


def test_status_word_is_clean_after_the_module(gpu_device):
    from opengaussian_amd import _lib
    torch.cuda.synchronize()
    assert _lib.lib().ogs_check_async_status() == 0
