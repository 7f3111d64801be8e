"""GPU: the stream contract.  Every launching function of include/*.h takes a `void* stream` and every Python wrapper hands it
torch's current stream; here every public entry point, and every C entry point with a memset, a copy or several launches, runs on
a fresh side stream behind a long delay (tests/stream_harness.py), off the legacy default stream that forgives a launch on the
wrong stream.  The table is tests/stream_contract_cases.py; the delay and the host times it is derived from are
profiles/stream_contract.json, with the host times of the self-test hook cases in profiles/stream_contract_hooks.json."""
import pytest
import torch

from tests import stream_contract_cases as table
from tests import stream_harness as H

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in table.CASES]
HOOK_NAMES = [c.name for c in table.HOOK_CASES]          # self-test hooks: the same run, host times in a profile of their own


@pytest.fixture(scope="module")
def delay_ms(gpu_device):
    """the delay of the profile, checked against its own rule -- over the host times of the table's cases and of the hook cases --
    and against the clock of this session"""
    prof = H.load_profile()
    assert set(prof["host_ms"]) == set(NAMES), "profiles/stream_contract.json was measured for another table"
    assert set(H.load_hook_profile()["host_ms"]) == set(HOOK_NAMES), "profiles/stream_contract_hooks.json: other hook cases"
    host_ms = H.all_host_ms()
    required = H.required_delay_ms(host_ms)
    assert required >= H.MIN_DELAY_MS and required >= H.DELAY_FACTOR * max(host_ms.values())
    assert prof["delay_ms"] >= required, (prof["delay_ms"], required)
    measured = H.measured_delay_ms(prof["delay_ms"])
    print("delay", prof["delay_ms"], "ms asked,", round(measured, 1), "ms measured,", required, "ms required")
    assert measured >= required, f"the calibrated delay ran {measured:.1f} ms, {required:.1f} ms are required"
    return float(prof["delay_ms"])


# ---- a, b, c: every entry point behind the delay ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES + HOOK_NAMES)
def test_call_on_a_side_stream_behind_a_delay(gpu_device, delay_ms, name):
    case = table.ALL_BY_NAME[name]
    v = H.run_behind_delay(case, gpu_device, delay_ms)
    print(name, "equal", v.equal, "returned before the delay ended", v.returned_before_delay_ended, "host ms", round(v.host_ms, 2),
          v.detail)
    assert v.decoy_is_valid, "the decoy must be valid input of the same shapes and ranges"
    assert v.decoy_differs, (f"outputs {v.same_for_both} are the same for both draws, the table lists {tuple(case.fixed_outputs)}: "
                             "every other output must tell a stray launch from a right one")
    assert v.default_stream_ran_ahead, "the side stream held the default stream back: a stray launch would not have shown"
    assert set(case.reaches) <= v.called, f"declared but not called: {sorted(set(case.reaches) - v.called)}"
    assert v.equal, v.detail
    assert v.status_word_clean
    if case.asserts_async:
        assert v.returned_before_delay_ended, f"documented as asynchronous ({case.sentence}) but the call waited for the stream"


# ---- d: two streams interleaved ---------------------------------------------------------------------------------------------------
INTERLEAVED = ["raster_tiny_forward", "raster_streaming_deferred", "render_kept_reblend", "wide_kmeans", "knn_lists",
               "c_radix_one_launch"]
ROUNDS = 8


def _snap(outs, s):
    with torch.cuda.stream(s):
        return [o.detach().clone() for o in outs]


@pytest.mark.parametrize("name", INTERLEAVED)
def test_two_streams_interleaved(gpu_device, delay_ms, name):
    """Two draws of one case, A on s1 and B on s2, 8 rounds alternating with no host synchronisation between the calls, each
    stream behind its own delay in round 0 (until it ends, A's buffers hold B's inputs and the other way round).  Every result
    must be the serial default-stream result of its own draw.  What it looks for is state shared by the two streams (scratch,
    the read-back slot, the capacity hints, the status word) and work on the wrong stream.
    This test can only ever pass wrongly, never fail wrongly: a race it is meant to catch may happen not to bite in a given
    run, but a result that differs from the serial one is a defect."""
    from opengaussian_amd import _lib
    case = table.BY_NAME[name]
    dev = gpu_device
    preps = [case.build(dev), case.build(dev)]
    draws = [{k: v.to(dev) for k, v in p.inputs(seed).items()} for p, seed in zip(preps, (H.REAL_SEED, H.DECOY_SEED))]
    bufs = [{k: v.clone() for k, v in d.items()} for d in draws]
    want = []
    for p, b in zip(preps, bufs):
        H._dirty(p)
        p.run(b, None)                                           # warm-up, and the first call of a case that keeps state
        H._dirty(p)
        want.append(H._snapshot(p.run(b, None)))
    torch.cuda.synchronize()
    assert not H.same(want[0], want[1], case.compare)[0], "the two draws give the same result"
    for b, other in zip(bufs, reversed(draws)):
        for k in b:
            b[k].copy_(other[k])
    torch.cuda.synchronize()
    _lib.lib().ogs_check_async_status()
    streams = H.side_streams()
    for s, p, b, d in zip(streams, preps, bufs, draws):
        with torch.cuda.stream(s):
            H.delay(s, delay_ms)
            for k in b:
                b[k].copy_(d[k])
            H._dirty(p)
    got = [[], []]
    for _ in range(ROUNDS):
        for i in (0, 1):
            got[i].append(_snap(preps[i].run(bufs[i], streams[i]), streams[i]))
    torch.cuda.synchronize()
    for i in (0, 1):
        for r, outs in enumerate(got[i]):
            ok, detail = H.same(outs, want[i], case.compare)
            assert ok, f"stream {i + 1}, round {r}: {detail}"
    assert _lib.lib().ogs_check_async_status() == 0


def test_a_background_tiled_on_one_stream_is_not_handed_to_another(gpu_device, delay_ms):
    """rasterizer._BG_TILED caches the 3-wide background tiled over a fused pass's channels.  The tiling is a launch on the
    stream of the pass that first asks; a pass on ANOTHER stream that found the entry would read it with nothing ordering it
    behind that launch.  s1: delay, then a tiny fused pass (asynchronous: the tiling sits behind the delay); s2, at once: the
    same pass with the same settings.  Both must give the default-stream result, whose background tensor is another one."""
    from opengaussian_amd import rasterizer as R
    dev = gpu_device
    P = 200
    sc = {k: v.to(dev) for k, v in table._scene(P, 5).items()}
    colour = (0.61, 0.17, 0.93)                                    # of this test alone: no stale block can hold it tiled

    def call(rs):
        with torch.no_grad():
            return R.rasterize_fused(sc["means3D"], torch.zeros(P, 3, device=dev), sc["opacities"], sc["shs"], sc["ins_feat"], rs,
                                     scales=sc["scales"], rotations=sc["rotations"])[0]
    want = call(table._settings(dev, colour)).clone()
    rs = table._settings(dev, colour)
    torch.cuda.synchronize()
    assert not torch.equal(want[3:], call(table._settings(dev, (0.0, 0.0, 0.0)))[3:]), "the background shows in no feature channel"
    s1, s2 = H.side_streams()
    with torch.cuda.stream(s1):
        H.delay(s1, delay_ms)
        first = call(rs)
        ev = torch.cuda.Event()
        ev.record(s1)
    with torch.cuda.stream(s2):
        second = call(rs)
    assert not ev.query(), "the pass on s1 was meant to be still behind its delay"
    torch.cuda.synchronize()
    assert torch.equal(first, want)
    assert torch.equal(second, want), "the pass on s2 read a background that s1 had not tiled yet"


# ---- e: negative controls: the harness can fail -------------------------------------------------------------------------------------
@pytest.mark.parametrize("module,name", [("rasterizer", "raster_tiny_forward"), ("knn", "knn_lists")])
def test_control_a_launch_on_stream_zero_is_seen(gpu_device, delay_ms, monkeypatch, module, name):
    """the wrapper's _stream() answers 0: its kernels run on the legacy default stream, which a non-blocking side stream does
    not hold back, read the decoy and write a result that is not the real one.  Every buffer involved is a valid allocation of
    the right size: a wrong answer, nothing else."""
    import importlib
    mod = importlib.import_module("opengaussian_amd." + module)
    monkeypatch.setattr(mod, "_stream", lambda: 0)
    v = H.run_behind_delay(table.BY_NAME[name], gpu_device, delay_ms)
    assert v.decoy_differs and v.default_stream_ran_ahead
    assert not v.equal, "work on stream 0 went unnoticed"


def test_control_a_hidden_synchronisation_is_seen(gpu_device, delay_ms, monkeypatch):
    from opengaussian_amd import kmeans
    real = kmeans.wide_assign

    def synced(*a, **kw):
        torch.cuda.current_stream().synchronize()
        return real(*a, **kw)
    monkeypatch.setattr(kmeans, "wide_assign", synced)
    v = H.run_behind_delay(table.BY_NAME["wide_kmeans"], gpu_device, delay_ms)
    assert v.equal, v.detail
    assert v.returned_before_delay_ended is False, "a synchronisation in front of a sync-free wrapper went unnoticed"
