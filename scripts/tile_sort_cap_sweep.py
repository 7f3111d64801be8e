"""The bucket cap of the one-wave depth sort: one-tile lists whose largest bucket is known, ranked inside their buckets against
the same lists under the LSD passes.

A launch with ONE list is one wave: its duration is the list's dependent chain, which is what the cap trades.  The lists have n
entries in tile (1, 1) of a 64 x 48 image (the scenes of tests/test_1d): keys 0x40000000 + (digit << 17) + low bits, a 25-bit
span (four LSD passes, as the bench scenes have), `big` entries in bucket 0 and the others dealt round over buckets 1 .. 255.

    rocprofv3 --kernel-trace -d DIR -o sweep -- python scripts/tile_sort_cap_sweep.py run
    python scripts/tile_sort_cap_sweep.py parse DIR          -> one JSON line: median us per (n, big, path)"""
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = (512, 1024)
BIGS = (8, 16, 32, 64, 128, 256)
PATHS = (("buckets", 1 << 20), ("lsd", 1))
REPS, SKIP = 10, 3


def keys_of(n, big, seed):
    rng = np.random.default_rng(seed)
    digit = np.concatenate([np.zeros(big, np.int64), 1 + np.arange(n - big) % 255])
    low = rng.permutation(1 << 17)[:n]
    return (0x40000000 + (digit << 17) + low)[rng.permutation(n)].astype(np.uint32)


def run():
    import torch
    from opengaussian_amd import _lib
    from tests import helpers
    from tests import test_1d_tile_depth_buckets_gpu as T
    dev = torch.device("cuda:0")
    lib = _lib.lib()
    for n in SIZES:
        for big in BIGS:
            z = keys_of(n, big, n + big).view(np.float32)
            sc, cam, _ = T._scene(z, n + big)
            inp = helpers.oracle_inputs(sc, cam, use_sh=True)
            for _, cap in PATHS:
                lib.ogs_raster_tile_sort_debug(cap)
                for _ in range(REPS):
                    helpers.hip_forward(inp, cam, T.BG, 3, dev)
                torch.cuda.synchronize()
    lib.ogs_raster_tile_sort_debug(0)


def parse(trace_dir):
    from kernel_trace_stats import durations
    per = durations(trace_dir)
    mine = [v for k, v in per.items() if "tile_depth_sort_kernel" in k]
    forwards = len(SIZES) * len(BIGS) * len(PATHS) * REPS
    assert len(mine) == 1 and len(mine[0]) % forwards == 0, [len(v) for v in mine]
    per_forward = len(mine[0]) // forwards                       # launches of the kernel per forward
    it = iter(mine[0])
    out = {"launches_per_forward": per_forward}
    for n in SIZES:
        for big in BIGS:
            for name, _ in PATHS:
                v = [next(it) for _ in range(REPS * per_forward)][SKIP * per_forward:]
                out[f"n{n}_big{big}_{name}"] = round(statistics.median(v), 2)
    print(json.dumps(out))


if __name__ == "__main__":
    run() if sys.argv[1] == "run" else parse(sys.argv[2])
