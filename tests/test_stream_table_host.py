"""CPU: the table of the stream contract tests (tests/stream_contract_cases.py) names every launcher of the C ABI.  Every
prototype of include/*.h with a `void* stream` parameter is reached by a case -- directly or through the wrapper the case calls;
tests/test_80_stream_contract_gpu.py checks on the GPU that the case really went through it -- or stands in the closed EXEMPT
dict with a reason."""
import os
import re

from tests import stream_contract_cases as table
from tests import stream_harness as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_EXEMPT = 6
HOOK = re.compile(r"^ogs_(selftest|prof)_|_debug$")


def test_the_header_scan_finds_the_launchers():
    protos = H.stream_prototypes()
    assert len(protos) >= 80, sorted(protos)
    for name in ("ogs_raster_forward_geometry", "ogs_knn_dbscan", "ogs_kmeans_wide_seed", "ogs_selftest_radix_sort",
                 "ogs_separation_loss", "ogs_refine_finalize", "ogs_densify_plan", "ogs_raster_backward_raw"):
        assert name in protos, name
    for name in ("ogs_version", "ogs_raster_geom_bytes", "ogs_raster_tile_sort_debug", "ogs_prof_enable", "ogs_check_async_status"):
        assert name not in protos, name


def test_every_launcher_is_named_by_a_case_or_exempt():
    protos = H.stream_prototypes()
    tabled = {n for c in table.CASES for n in c.reaches}
    named = tabled | {n for c in table.HOOK_CASES for n in c.reaches}
    missing = protos - named - set(table.EXEMPT)
    assert not missing, f"launchers no stream case reaches: {sorted(missing)}"
    # the hook cases are for self-test hooks alone: an entry point of the product is named by the table itself
    for n in sorted(named - tabled):
        assert HOOK.search(n), f"{n} is no hook: its case belongs in CASES"
    for c in table.HOOK_CASES:
        assert all(HOOK.search(n) for n in c.reaches) and c.level == "c", c.name
    assert not set(table.EXEMPT) & named, "exempt and named at once"
    assert set(table.EXEMPT) <= protos, "an exemption for something that is no launcher"


def test_exemptions_are_few_reasoned_and_hooks_only():
    assert len(table.EXEMPT) <= MAX_EXEMPT
    for name, reason in table.EXEMPT.items():
        assert isinstance(reason, str) and len(reason.split()) >= 5, name
        assert HOOK.search(name), f"{name} is neither a profiling nor a debug hook"


def test_every_name_in_the_table_is_bound():
    from opengaussian_amd import _lib
    protos = H.stream_prototypes()
    for c in table.ALL_CASES:
        assert c.reaches, c.name
        for n in c.reaches:
            assert n in _lib.SIGNATURES, (c.name, n)
            assert n in protos, f"{c.name}: {n} takes no stream"


def test_table_entries_are_complete():
    names = [c.name for c in table.ALL_CASES]
    assert len(set(names)) == len(names)
    for c in table.ALL_CASES:
        assert c.level in ("py", "c"), c.name
        if c.blocks_host:
            assert c.sentence, f"{c.name}: blocks_host needs the sentence that documents it"
        rules = c.compare if isinstance(c.compare, list) else [c.compare]
        if any(r != "bits" for r in rules):
            assert c.bar_from and "::" in c.bar_from, f"{c.name}: a tolerance names the test it is taken from"
            test_file = os.path.join(ROOT, c.bar_from.split("::")[0])
            assert os.path.exists(test_file), c.bar_from
            assert re.search(r"def " + re.escape(c.bar_from.split("::")[1].split("[")[0]) + r"\(", open(test_file).read()), c.bar_from
    # the paths the wrappers branch on, and the levels the issue lists
    for must in ("raster_tiny_forward", "raster_tiny_backward", "raster_streaming_blocking", "raster_streaming_deferred",
                 "render_kept_reblend", "c_raster_deferred_forward", "c_radix_one_launch"):
        assert must in table.BY_NAME, must
    assert sum(c.level == "c" for c in table.CASES) >= 10


def test_the_profile_covers_the_table_and_obeys_its_rule():
    prof = H.load_profile()
    assert set(prof["host_ms"]) == {c.name for c in table.CASES}
    assert all(v > 0 for v in prof["host_ms"].values())
    assert prof["delay_ms"] >= H.required_delay_ms(prof["host_ms"]) >= H.MIN_DELAY_MS
    # the hook cases: a profile entry each, and the one delay covers them as it covers the table's
    hooks = H.load_hook_profile()
    assert set(hooks["host_ms"]) == {c.name for c in table.HOOK_CASES}
    assert all(v > 0 for v in hooks["host_ms"].values())
    assert set(H.all_host_ms()) == {c.name for c in table.ALL_CASES}
    assert prof["delay_ms"] >= H.required_delay_ms(H.all_host_ms()) >= H.MIN_DELAY_MS


def test_the_gpu_file_skips_nothing():
    src = open(os.path.join(ROOT, "tests", "test_80_stream_contract_gpu.py")).read()
    assert "skip" not in src.replace("skips", "") and "xfail" not in src
