"""CPU: resources of the per-tile depth sort (binning.hip::tile_depth_sort_kernel) as hipcc reports them for gfx950.

The kernel keeps its ranking state in registers (kTileSortItems keys, values and ranks per lane, indexed only by unrolled
loops) and its LDS plan is fixed: 4 wave histograms + digit starts + digit bases (256 words each), 4 scan words, 2 reduction
words, the workgroup's 4 tile ranges and kTileSortCap keys + values (the waves' digit match masks alias those).  A dynamically indexed register array would land in scratch; a larger LDS footprint
would cost workgroups per CU."""
import os
import re
import subprocess




def _remarks(tmp_path):
    from opengaussian_amd import build
    src = os.path.join(build.CSRC, "binning.hip")
    cmd = [build.hipcc(), *build.COMMON, *build.EXTRA.get("binning.hip", []), "-c", src, "-o", str(tmp_path / "binning.o"),
           "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return r.stderr


def test_tile_depth_sort_has_no_scratch_and_the_planned_lds(tmp_path):
    from opengaussian_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    cap = int(_lib.lib().ogs_raster_tile_sort_capacity(1))
    assert int(_lib.lib().ogs_raster_tile_sort_capacity(0)) * 4 == cap       # one wave: a quarter of the space
    out = _remarks(tmp_path)
    blocks = re.split(r"remark: Function Name: ", out)
    mine = [b for b in blocks if b.startswith("_ZN3ogs") and "tile_depth_sort_kernel" in b.split()[0]]
    assert len(mine) == 1, [b.split()[0] for b in blocks[1:]]
    field = lambda name: int(re.search(name + r": (\d+)", mine[0]).group(1))
    assert field(r"ScratchSize \[bytes/lane\]") == 0
    assert field("VGPRs Spill") == 0
    assert field(r"LDS Size \[bytes/block\]") == 4 * (4 * 256 + 256 + 256 + 4 + 2 + 2 * 4 + 2 * cap)
