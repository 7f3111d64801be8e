"""CPU: where the kernels of the sorted-box walk (csrc/knn_boxes.h) are compiled, and their resources as hipcc reports them for
gfx950.

The K-nearest search is ONE set of four code objects (list sizes 4 / 8 / 16 / 32), all of them in knn_search.hip: knn_neighbors.hip and
knn_query.hip launch it through knn_launch_search and hold no copy.  The search and the radius walk (knn_radius.hip) keep their
lists and counters in registers and stage one box in LDS: no scratch, the planned LDS, and at least the waves per SIMD they had
before the search's lane set-up and bound moved into KnnLane -- 8, 8, 5, 2 and 5, 7, 8, read from the
commit before that move with the command below.  No VGPR count is pinned: DESIGN.md sections 6n and 6s carry those and name the compiler they rest on."""
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

FILES = ("knn_search.hip", "knn_radius.hip", "knn_neighbors.hip", "knn_query.hip")


def _functions(tmp, name):
    """{mangled name: remark block} of the kernels hipcc reports for csrc/<name>"""
    from opengaussian_amd import build
    cmd = [build.hipcc(), *build.COMMON, *build.EXTRA.get(name, []), "-c", os.path.join(build.CSRC, name), "-o",
           str(tmp / name.replace(".hip", ".o")), "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    blocks = re.split(r"remark: Function Name: ", r.stderr)[1:]
    return {b.split()[0]: b for b in blocks}


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("knn_box_resources")
    with ThreadPoolExecutor(max_workers=len(FILES)) as ex:
        return dict(zip(FILES, ex.map(lambda f: _functions(tmp, f), FILES)))


def _field(block, name):
    return int(re.search(name + r": (\d+)", block).group(1))


def _check(block, lds, waves):
    assert _field(block, r"ScratchSize \[bytes/lane\]") == 0
    assert _field(block, "VGPRs Spill") == 0
    assert _field(block, r"LDS Size \[bytes/block\]") == lds
    assert _field(block, r"Occupancy \[waves/SIMD\]") >= waves


def test_the_search_kernel_is_compiled_once(remarks):
    where = {f: sorted(n for n in fns if "knn_search_kernel" in n) for f, fns in remarks.items()}
    assert len(where["knn_search.hip"]) == 4, where
    assert where["knn_neighbors.hip"] == [] and where["knn_query.hip"] == [] and where["knn_radius.hip"] == [], where


@pytest.mark.parametrize("slots,waves", [(4, 8), (8, 8), (16, 5), (32, 2)])
def test_search_kernel_resources(remarks, slots, waves):
    mine = [b for n, b in remarks["knn_search.hip"].items() if f"knn_search_kernelILi{slots}EE" in n]
    assert len(mine) == 1, sorted(remarks["knn_search.hip"])
    _check(mine[0], 1024, waves)           # x, y, z and id of one box


# template arguments <MODE, TAGS> as the mangled name spells them
@pytest.mark.parametrize("which,args,lds,waves", [("count with tags", "ILi0ELb1EE", 1024, 5),       # x, y, z, tag
                                                  ("count without tags", "ILi0ELb0EE", 768, 7),     # x, y, z
                                                  ("link", "ILi1ELb1EE", 1280, 8)])                 # x, y, z, id, tag
def test_radius_walk_resources(remarks, which, args, lds, waves):
    mine = [b for n, b in remarks["knn_radius.hip"].items() if "radius_walk_kernel" + args in n]
    assert len(mine) == 1, (which, sorted(remarks["knn_radius.hip"]))
    _check(mine[0], lds, waves)
    assert sum("radius_walk_kernel" in n for n in remarks["knn_radius.hip"]) == 3
