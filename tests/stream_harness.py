"""The stream contract harness: run one entry point on a fresh side stream that sits behind a long delay and see whether it
(a) still computes what it computes on the default stream and (b) comes back to the host before the delay has run out.

Why a delay: the legacy default stream orders itself against every blocking stream, and all of the suite's other GPU tests launch
on it, so a memset, copy or kernel issued on stream 0 instead of the caller's stream gives the right bytes there.  torch's side
streams are NON-blocking: stream 0 does not wait for them.  Here the real inputs reach their buffers only at the END of the side
stream's delay; until then the buffers hold a DECOY (valid input of the same shapes and ranges from another seed).  Work that
strays to another stream runs at once, reads the decoy -- or writes what the caller's stream overwrites later -- and the result
is the decoy's, not the real one.  A stray launch gives a wrong answer, never an out-of-bounds access.

The flags alone do not make that so.  A process has a few hardware queues (4 by default) and the runtime maps its streams onto
them; two streams that share a queue run in submission order, and work that strayed to the default stream would then wait for
the side stream's delay like work in the right place.  So the two side streams of a session are chosen once by a probe
(`side_streams`: a short spin on one must not hold back a fill on the default stream or on the other), and every run carries a
canary: a fill on the default stream, issued in front of the call, has finished while the delay still runs
(`Verdict.default_stream_ran_ahead`).  The issue asks for a fresh stream per case; a probed stream reused per session is what
keeps the number of streams down, and the canary holds for every run.

The table of cases is tests/stream_contract_cases.py; the tests are tests/test_80_stream_contract_gpu.py (GPU) and
tests/test_stream_table_host.py (CPU: every `void* stream` prototype of include/*.h is named by a case or exempted).

`python -m tests.stream_harness --measure` (on the GPU) times every tabled call on the host after one warm-up call and writes
profiles/stream_contract.json: the host times and the delay derived from them (at least 10 x the largest, at least 50 ms).
`python -m tests.stream_harness --table` prints the table: every case with its blocks_host flag and the sentence it is taken from.

The cases of self-test hooks (HOOK_CASES of the table module) run through the same tests as the table's own.  Their host times
are profiles/stream_contract_hooks.json, which `--measure` writes as well (and `--measure-hooks` alone); the one delay, that of
profiles/stream_contract.json, must be at least 10 x the largest host time of EITHER file."""
from __future__ import annotations

import contextlib
import json
import os
import time
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "stream_contract.json")
HOOK_PROFILE = os.path.join(ROOT, "profiles", "stream_contract_hooks.json")
REAL_SEED, DECOY_SEED = 1234, 4321
MIN_DELAY_MS = 50.0
DELAY_FACTOR = 10.0
DIRTY_BYTE = 0xA5


# ---- what a case is ---------------------------------------------------------------------------------------------------------------
@dataclass
class Prepared:
    """One case, built on the device.
    inputs(seed) -> {name: CPU tensor}: every draw has the same names, shapes and dtypes, finite floats and in-range indices.
    run(bufs, stream) -> list of tensors: the call on the device buffers `bufs` (same names).  stream None: the default stream.
        Otherwise everything the case launches goes under ``torch.cuda.stream(stream)`` (``on(stream)``), except a backward,
        which is called from default-stream context with its upstream gradient produced on `stream`.
    out / tmp: caller-owned pure outputs and scratch of a C-ABI case, dirtied with 0xA5 on the stream before the call;
    clear: outputs whose contract says "the caller clears it", zeroed on the stream after that.
    check(outputs) -> None or a message: what the outputs of ONE call must satisfy among themselves (after synchronisation)."""
    inputs: Callable[[int], Dict[str, torch.Tensor]]
    run: Callable[[Dict[str, torch.Tensor], Optional[torch.cuda.Stream]], Sequence[torch.Tensor]]
    out: List[torch.Tensor] = field(default_factory=list)
    tmp: List[torch.Tensor] = field(default_factory=list)
    clear: List[torch.Tensor] = field(default_factory=list)
    check: Optional[Callable[[Sequence[torch.Tensor]], Optional[str]]] = None


@dataclass
class Case:
    """A row of the table.  reaches: the C entry points with a `void* stream` the call goes through (checked on the GPU against
    what the call really called).  level: "py" (a public wrapper) or "c" (through _lib.lib() with caller-owned buffers).
    blocks_host: the call hands a value to the host, `sentence` is where that is documented; otherwise `sentence` is where the
    call is documented as asynchronous, and None means no document says either (only the result is checked).
    compare: "bits", or (rtol, atol, relative-to-the-largest-entry bar) with `bar_from` naming the test the bar is taken from, or a
    list of those, one per output.
    fixed_outputs: indices of the outputs that are the same for both draws -- they do not depend on the draw (the geometry of a
    frozen model, say) or the two draws agree on them (a count) -- and so cannot show a stray launch: the blind spots, on
    record.  EVERY other output must differ between the two draws, and a listed one must not."""
    name: str
    build: Callable[[torch.device], Prepared]
    reaches: Sequence[str]
    level: str = "py"
    blocks_host: bool = False
    sentence: Optional[str] = None
    compare: object = "bits"
    bar_from: Optional[str] = None
    fixed_outputs: Sequence[int] = ()

    @property
    def asserts_async(self) -> bool:
        return not self.blocks_host and self.sentence is not None


@dataclass
class Verdict:
    equal: bool
    returned_before_delay_ended: bool
    status_word_clean: bool
    decoy_is_valid: bool            # same names / shapes / dtypes as the real draw, finite
    decoy_differs: bool             # output by output, want != want_decoy under the case's own comparison, except Case.fixed_outputs
    called: frozenset               # the stream-taking C entry points the call went through
    host_ms: float
    detail: str = ""
    default_stream_ran_ahead: bool = True   # work on the default stream finished while the delay ran: a stray launch would show
    same_for_both: tuple = ()               # the outputs on which want == want_decoy (held against Case.fixed_outputs)


def on(stream):
    """context of a case's launches: the side stream, or nothing for the default stream"""
    return contextlib.nullcontext() if stream is None else torch.cuda.stream(stream)


# ---- the delay ----------------------------------------------------------------------------------------------------------------------
_CYCLES_PER_MS = None


def load_profile() -> dict:
    with open(PROFILE) as f:
        return json.load(f)


def load_hook_profile() -> dict:
    with open(HOOK_PROFILE) as f:
        return json.load(f)


def all_host_ms() -> Dict[str, float]:
    """the host times of both profiles: what the one delay is held against"""
    return {**load_profile()["host_ms"], **load_hook_profile()["host_ms"]}


def required_delay_ms(host_ms: Dict[str, float]) -> float:
    return max(MIN_DELAY_MS, DELAY_FACTOR * max(host_ms.values()))


def _timed_sleep(cycles: int) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    torch.cuda._sleep(int(cycles))
    b.record()
    b.synchronize()
    return float(a.elapsed_time(b))


def cycles_per_ms() -> float:
    """spin cycles of torch.cuda._sleep per millisecond, measured once per session with events"""
    global _CYCLES_PER_MS
    if _CYCLES_PER_MS is None:
        _timed_sleep(1_000_000)                                  # first launch
        n = 20_000_000
        ms = min(_timed_sleep(n) for _ in range(3))
        _CYCLES_PER_MS = n / max(ms, 1e-3)
    return _CYCLES_PER_MS


def delay(stream, ms: Optional[float] = None):
    """enqueue plain torch work of at least `ms` milliseconds on `stream` (default: the delay of the profile)"""
    ms = load_profile()["delay_ms"] if ms is None else ms
    with torch.cuda.stream(stream):
        torch.cuda._sleep(int(1.15 * ms * cycles_per_ms()))


def measured_delay_ms(ms: Optional[float] = None) -> float:
    """how long the delay really takes on an otherwise idle device (events around it)"""
    ms = load_profile()["delay_ms"] if ms is None else ms
    s = side_streams()[0]
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(s)
    delay(s, ms)
    b.record(s)
    b.synchronize()
    return float(a.elapsed_time(b))


def runs_beside(s, other=None, ms: float = 5.0) -> bool:
    """True when work on `other` (None: the legacy default stream) is NOT held back by work queued on `s`.  A process has a
    few hardware queues and the runtime maps its streams onto them; two streams that share one run in submission order,
    whatever their flags say, and a launch that strays from `s` to such a stream would wait for the delay like a right one.
    Probe: a 5 ms spin on `s`, then a fill on `other`; the fill must be done while the spin still runs."""
    torch.cuda.synchronize()
    cycles = int(ms * cycles_per_ms())
    with torch.cuda.stream(s):
        torch.cuda._sleep(cycles)
        spun = torch.cuda.Event()
        spun.record(s)
    with on(other):
        torch.zeros(16, device="cuda")
        filled = torch.cuda.Event()
        filled.record()
    filled.synchronize()
    beside = not spun.query()
    torch.cuda.synchronize()
    return beside


def _independent_stream(*others, tries: int = 16):
    """a side stream that holds back neither the legacy default stream nor any of `others`"""
    for _ in range(tries):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            torch.zeros(16, device="cuda")                       # first use: the runtime settles the stream's queue
        if runs_beside(s) and all(runs_beside(s, o) and runs_beside(o, s) for o in others):
            return s
    raise RuntimeError("no side stream runs beside the default stream: the process has too few hardware queues")


_SIDE_STREAMS = None


def side_streams():
    """(s1, s2): the two side streams every test of the session works on, probed once -- neither holds back the default stream
    or the other.  Only these two and the default stream ever carry a test's work; the probe itself looks at up to 16
    candidates per stream, once per process, with a 5 ms spin each (the one departure from "no more than three streams":
    torch offers no way to ask which hardware queue a stream got, so candidates have to be tried)."""
    global _SIDE_STREAMS
    if _SIDE_STREAMS is None:
        cycles_per_ms()
        s1 = _independent_stream()
        _SIDE_STREAMS = (s1, _independent_stream(s1))
    return _SIDE_STREAMS


# ---- comparison ------------------------------------------------------------------------------------------------------------------
def _bits(t: torch.Tensor) -> torch.Tensor:
    t = t.detach().contiguous()
    if t.dtype in (torch.float32,):
        return t.view(torch.int32)
    if t.dtype in (torch.float64,):
        return t.view(torch.int64)
    if t.dtype is torch.bool:
        return t.view(torch.uint8)
    return t


def same(got, want, compare) -> (bool, str):
    """bit patterns, or the family's bar: |got - want| <= atol + rtol |want| element by element when bar is None, else
    max |got - want| <= bar * max |want|"""
    if len(got) != len(want):
        return False, f"{len(got)} outputs against {len(want)}"
    per_output = compare if isinstance(compare, list) else [compare] * len(got)
    if len(per_output) != len(got):
        return False, f"{len(got)} outputs, {len(per_output)} comparison rules"
    for i, (g, w, compare) in enumerate(zip(got, want, per_output)):
        if g.shape != w.shape or g.dtype != w.dtype:
            return False, f"output {i}: {tuple(g.shape)} {g.dtype} against {tuple(w.shape)} {w.dtype}"
        if compare == "bits" or not g.is_floating_point():
            if not torch.equal(_bits(g), _bits(w)):
                return False, f"output {i}: bits differ in {int((_bits(g) != _bits(w)).sum())} of {g.numel()} elements"
            continue
        rtol, atol, bar = compare
        g64, w64 = g.detach().double(), w.detach().double()
        if not bool(torch.isfinite(g64).all()):
            return False, f"output {i}: not finite"
        d = (g64 - w64).abs()
        if bar is not None:
            if g.numel() and float(d.max()) > bar * float(w64.abs().max()):
                return False, f"output {i}: off by {float(d.max()):.3e}, largest entry {float(w64.abs().max()):.3e}, bar {bar}"
        elif g.numel() and not bool((d <= atol + rtol * w64.abs()).all()):
            return False, f"output {i}: off by {float(d.max()):.3e} (rtol {rtol}, atol {atol})"
    return True, ""


def same_outputs(a, b, compare) -> List[int]:
    """indices of the outputs on which two results agree under the case's comparison"""
    per_output = compare if isinstance(compare, list) else [compare] * len(a)
    return [i for i, (x, y, c) in enumerate(zip(a, b, per_output)) if same([x], [y], [c])[0]]


def _snapshot(outs) -> List[torch.Tensor]:
    return [o.detach().clone() for o in outs]


# ---- which C entry points a call went through ------------------------------------------------------------------------------------
class _Recorder:
    """stands in for the loaded library: every attribute is the library's own, calls of ogs_* functions are noted"""

    def __init__(self, real, seen):
        object.__setattr__(self, "_real", real)
        object.__setattr__(self, "_seen", seen)

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("ogs_"):
            return fn
        seen = self._seen

        def call(*a):
            seen.add(name)
            return fn(*a)
        return call


@contextlib.contextmanager
def recording():
    from opengaussian_amd import _lib
    real, seen = _lib.lib(), set()
    _lib._lib = _Recorder(real, seen)
    try:
        yield seen
    finally:
        _lib._lib = real


def stream_prototypes() -> set:
    """the names of include/*.h prototypes with a `void* stream` parameter"""
    import re
    proto = re.compile(r"^\s*(?:int|size_t)\s+(ogs_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", re.M | re.S)
    names = set()
    inc = os.path.join(ROOT, "include")
    for fn in sorted(os.listdir(inc)):
        if fn.endswith(".h"):
            text = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, fn)).read(), flags=re.S)
            for name, params in proto.findall(text):
                if re.search(r"void\s*\*\s*stream\b", params):
                    names.add(name)
    return names


# ---- the run ----------------------------------------------------------------------------------------------------------------------
def _valid_pair(real, decoy) -> bool:
    if set(real) != set(decoy):
        return False
    for k, r in real.items():
        d = decoy[k]
        if r.shape != d.shape or r.dtype != d.dtype:
            return False
        if d.is_floating_point() and not bool(torch.isfinite(d).all() and torch.isfinite(r).all()):
            return False
    return True


def _dirty(prep: Prepared):
    for t in list(prep.out) + list(prep.tmp):
        t.view(-1).view(torch.uint8).fill_(DIRTY_BYTE)
    for t in prep.clear:
        t.zero_()


def prepare(case: Case, dev):
    """build the case, stage both draws on the device, compute want / want_decoy on the default stream (this is also the warm-up
    call); leaves the decoy in the input buffers.  Returns (prep, bufs, staged real inputs, want, want_decoy, decoy_is_valid)."""
    prep = case.build(dev)
    real, decoy = prep.inputs(REAL_SEED), prep.inputs(DECOY_SEED)
    valid = _valid_pair(real, decoy)
    real_dev = {k: v.to(dev) for k, v in real.items()}
    decoy_dev = {k: v.to(dev) for k, v in decoy.items()}
    bufs = {k: v.clone() for k, v in real_dev.items()}
    _dirty(prep)
    want = _snapshot(prep.run(bufs, None))
    for k in bufs:
        bufs[k].copy_(decoy_dev[k])
    _dirty(prep)
    want_decoy = _snapshot(prep.run(bufs, None))
    torch.cuda.synchronize()
    return prep, bufs, real_dev, want, want_decoy, valid


def run_behind_delay(case: Case, dev, delay_ms: Optional[float] = None) -> Verdict:
    from opengaussian_amd import _lib
    prep, bufs, real_dev, want, want_decoy, valid = prepare(case, dev)
    blind = same_outputs(want_decoy, want, case.compare) if len(want) == len(want_decoy) else []
    differs = len(blind) < len(want) and set(blind) == set(case.fixed_outputs)
    _lib.lib().ogs_check_async_status()                          # whatever earlier tests left: not this call's
    s = side_streams()[0]
    # one warm-up call on the side stream itself (its allocator pool, per-stream scratch), on the decoy, without a delay
    with torch.cuda.stream(s):
        _dirty(prep)
    prep.run(bufs, s)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        delay(s, delay_ms)
        for k in bufs:
            bufs[k].copy_(real_dev[k])
        _dirty(prep)
        ev = torch.cuda.Event()
        ev.record(s)
    # the canary: a fill on the default stream, in front of whatever the call may let stray there, is done while the delay runs
    torch.zeros(16, device=dev)
    canary = torch.cuda.Event()
    canary.record()
    canary.synchronize()
    ahead = not ev.query()
    with recording() as seen:
        t0 = time.perf_counter()
        got = prep.run(bufs, s)
        early = not ev.query()
        host_ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    clean = _lib.lib().ogs_check_async_status() == 0
    equal, detail = same(list(got), want, case.compare)
    if equal and prep.check is not None:
        detail = prep.check(list(got)) or ""
        equal = not detail
    return Verdict(equal, early, clean, valid, differs, frozenset(seen), host_ms, detail, ahead, tuple(blind))


def host_time_ms(case: Case, dev) -> float:
    """host wall time of the call on the default stream, after one warm-up call (prepare() makes two)"""
    prep, bufs, real_dev, _, _, _ = prepare(case, dev)
    _dirty(prep)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    prep.run(bufs, None)
    ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    return ms


def measure(path=PROFILE):
    from tests import stream_contract_cases as table
    dev = torch.device("cuda:0")
    return write_profile({c.name: round(host_time_ms(c, dev), 3) for c in table.CASES}, path)


def measure_hooks(path=HOOK_PROFILE):
    """the host times of the hook cases, taken as measure() takes the table's; the delay stays that of profiles/stream_contract.json"""
    from tests import stream_contract_cases as table
    dev = torch.device("cuda:0")
    doc = {"what": "host wall time (ms) of every hook case (HOOK_CASES) on the default stream after one warm-up call; the delay of "
                   "profiles/stream_contract.json covers these too.  Written by `python -m tests.stream_harness --measure-hooks`",
           "device": torch.cuda.get_device_name(0),
           "host_ms": {c.name: round(host_time_ms(c, dev), 3) for c in table.HOOK_CASES}}
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return doc


def write_profile(host: Dict[str, float], path=PROFILE):
    want = required_delay_ms(host)
    delay_ms = float(50 * -(-want // 50))                        # rounded up to 50 ms
    doc = {"what": "host wall time (ms) of every tabled call on the default stream after one warm-up call, and the delay the "
                   "stream contract tests put in front of each call: at least 10 x the largest of them, at least 50 ms.  "
                   "Written by `python -m tests.stream_harness --measure`, with the wrappers as they stand in the tree",
           "device": torch.cuda.get_device_name(0), "largest_host_ms": max(host.values()),
           "required_delay_ms": want, "delay_ms": delay_ms, "measured_delay_ms": round(measured_delay_ms(delay_ms), 2),
           "host_ms": host}
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return doc


def print_table():
    """the table as markdown: case, level, blocks_host, the sentence the flag is taken from, the entry points it reaches"""
    from tests import stream_contract_cases as table
    print("| case | level | blocks_host | documented by | reaches |\n|---|---|---|---|---|")
    for c in table.ALL_CASES:
        print(f"| {c.name} | {c.level} | {c.blocks_host} | {c.sentence or '(neither documented: result only)'} | "
              f"{', '.join(c.reaches)} |")
    print("\nexempt:")
    for name, reason in table.EXEMPT.items():
        print(f"- {name}: {reason}")


if __name__ == "__main__":
    import sys
    if "--table" in sys.argv:
        print_table()
    if "--measure" in sys.argv:
        out = sys.argv[sys.argv.index("--measure") + 1] if len(sys.argv) > sys.argv.index("--measure") + 1 else PROFILE
        d = measure(out)
        print(json.dumps({k: d[k] for k in ("largest_host_ms", "required_delay_ms", "delay_ms", "measured_delay_ms")}))
        print(json.dumps(measure_hooks(HOOK_PROFILE if out == PROFILE else out[:-5] + "_hooks.json")["host_ms"]))
    if "--measure-hooks" in sys.argv:
        i = sys.argv.index("--measure-hooks")
        print(json.dumps(measure_hooks(sys.argv[i + 1] if len(sys.argv) > i + 1 else HOOK_PROFILE)["host_ms"]))
