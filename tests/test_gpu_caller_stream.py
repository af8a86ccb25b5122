"""The fit on a caller's stream (sgl_set_stream, Context.set_stream) and the all-reduce hook on it.

The contract under test is the one of include/singlet_hip.h ("Collective hook for cell-sharded runs"): after
set_stream(S) ALL work of a resident call goes to S, host reads wait for S, the library makes no host synchronisation
before the hook and the hook enqueues on S; on the private stream (handle 0 / None) the library synchronises first and the
hook must have finished when it returns.

The stall.  A race does not show by chance, so every library call is preceded by a short spin of ONE thread at the head of
the stream under test (torch.cuda._sleep, calibrated once per session with two events; a chain of small matmuls where torch
lacks it).  Work the library launched on any other stream, or read on the host without waiting for the stream, overtakes the
spin, sees stale data, and the bits differ.  The stall is STALL_MS = 4 x the longest host-side return of an asynchronous step
call, never above 100 ms.  Measured on an MI355X on the private stream without a stall, every fit run twice in one process,
4 iterations each (3 at 70 000 cells); ms per call, the longest of the first iterations / the longest of the later ones:

    shape, k               step_begin      step_h          step_scale_h    step_w
    300 x 1000, k = 8      0.015 / 0.016   2.260 / 0.050   0.018 / 0.013   0.036 / 0.030
    300 x 1000, k = 50     0.007 / 0.008   1.308 / 0.040   0.018 / 0.011   0.029 / 0.026
    300 x 1000, k = 100    0.006 / 0.013   1.742 / 0.063   0.015 / 0.011   0.054 / 0.050
    300 x 1000, k = 136    0.006 / 0.016   1.181 / 0.072   0.015 / 0.010   0.052 / 0.050
    257 x 700, k = 30      0.005 / 0.018   0.029 / 0.035   0.012 / 0.012   0.025 / 0.029
    1500 x 70000, k = 24   0.016 / 0.007   0.062 / 0.039   0.016 / 0.010   0.701 / 0.026

The first step_h at a rank in a process takes 1.2 - 2.3 ms (the same fit run again in that process: 0.03 - 0.05 ms) and the
first step_w at 70 000 cells 0.7 ms both times; every later call returns within 0.072 ms.  The longest of all is 2.260 ms,
so STALL_MS = 4 x 2.260 = 9.04: a fit of 4 iterations through the step API carries some 25 stalls, 0.23 s.

test_the_stall_outlasts_an_asynchronous_call is the one place where the stall checks itself: after a stall and step_begin
(one device-to-device hipMemcpyAsync) the stream is still busy when the call returns.

References: (a) the same call sequence on the private stream without stalls, bit for bit (the fit is deterministic:
fixed-order reductions); (b) for the fits the oracle, at 1e-9 relative Frobenius for W, d and H with identical zero patterns.
Two processes cannot share a stream, so the second shard of the hook tests is a mirror: one context holds A with
ncells_total = 2 n and the hook doubles the buffer -- the exact all-reduce of two identical shards -- against the oracle's fit
of [A | A].

Every test creates its own Context and leaves it on its private stream; torch's current stream changes only inside
`with torch.cuda.stream(S)`.  torch is imported inside the tests: the first of them pays its device initialisation.  Every
test brings torch up (the calibrated stall) BEFORE it creates its first context: run alone, with the library the first user
of the GPU in the process and torch imported after it, this file saw torch's first kernel launch fail with "no ROCm-capable
device is detected" (a torch build that ships its own HIP runtime next to the system's one); torch first, or torch after
the suite's other GPU tests, works.
"""
import contextlib
import ctypes

import numpy as np
import pytest

from conftest import rel_fro, same_zero_pattern, to_dgc

pytestmark = pytest.mark.gpu
STALL_MS = 9.04
TOL = 1e-9
L1 = 0.01
DEV = 0
STEP_CALLS = (("step_begin", ()), ("step_h", (L1, 0.0)), ("step_scale_h", ()), ("step_w", (L1, 0.0)), ("step_scale_w", ()))
_CACHE = {}


def cached(key, make):
    """References are computed once, shared, and never written to."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ---------------------------------------------------------------------------------------------------------- the stall
class Stall:
    """stall(stream): a spin of STALL_MS at the tail of `stream`'s queue.  Calibrated once per session."""

    def __init__(self, torch):
        self.torch = torch
        assert 0.0 < STALL_MS <= 100.0
        self.sleep = getattr(torch.cuda, "_sleep", None)
        if self.sleep is not None:
            self.unit = lambda count: self.sleep(int(count))
            probe = 2_000_000
        else:
            a = torch.ones((256, 256), device="cuda:%d" % DEV)

            def chain(count):
                for _ in range(int(count)):
                    torch.mm(a, a)
            self.unit = chain
            probe = 200
        self.unit(probe)                                   # code object load, first launch
        torch.cuda.synchronize(DEV)
        per_ms = max(probe / self._time(probe) for _ in range(3))   # the fastest reading: the most units per ms ...
        self.count = int(np.ceil(per_ms * STALL_MS))
        ms = self._time(self.count)
        if ms < STALL_MS:                                  # ... and a spin that still came out short is lengthened
            self.count = int(np.ceil(self.count * 1.1 * STALL_MS / ms))
            ms = self._time(self.count)
        assert STALL_MS <= ms <= 100.0, "the spin is not calibrated: %d units took %.3f ms" % (self.count, ms)
        self.measured_ms = ms

    def _time(self, count):
        e0, e1 = self.torch.cuda.Event(enable_timing=True), self.torch.cuda.Event(enable_timing=True)
        e0.record()
        self.unit(count)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def __call__(self, stream):
        with self.torch.cuda.stream(stream):
            self.unit(self.count)


def the_stall():
    import torch
    return cached("stall", lambda: Stall(torch))


class Stalled:
    """A context whose every call is preceded by a stall of the stream it launches on."""

    def __init__(self, c, stream):
        self._c, self._stream, self._stall = c, stream, the_stall()

    def __getattr__(self, name):
        f = getattr(self._c, name)
        if not callable(f):
            return f

        def call(*a, **kw):
            self._stall(self._stream)
            return f(*a, **kw)
        return call


@contextlib.contextmanager
def contexts(sa, n=1):
    """n fresh contexts; whatever happens they go back to their private stream before they are closed."""
    the_stall()                                            # torch first: see the module's last paragraph
    cs = [sa.Context(DEV) for _ in range(n)]
    try:
        yield cs if n > 1 else cs[0]
    finally:
        for c in cs:
            if c._h:
                try:
                    c.set_stream(None)
                finally:
                    c.close()


@contextlib.contextmanager
def caller_stream(*cs):
    """A fresh torch stream S, current for torch inside the block, with the contexts on it; they leave it at the end."""
    import torch
    the_stall()                                            # calibrated on the default stream, before S exists
    S = torch.cuda.Stream(device=DEV)
    try:
        with torch.cuda.stream(S):
            for c in cs:
                c.set_stream(S.cuda_stream)
            yield S
    finally:
        for c in cs:
            if c._h:
                c.set_stream(None)
        S.synchronize()


def bits_differ(got, want, path=""):
    """Names of the leaves of two nested results (dicts, tuples, arrays, numbers) that are not the same bits."""
    if isinstance(want, dict):
        if not isinstance(got, dict) or sorted(got) != sorted(want):
            return [path + ": keys"]
        return [d for key in sorted(want) for d in bits_differ(got[key], want[key], "%s.%s" % (path, key))]
    if isinstance(want, (tuple, list)):
        if not isinstance(got, (tuple, list)) or len(got) != len(want):
            return [path + ": length"]
        return [d for q, (g, w) in enumerate(zip(got, want)) for d in bits_differ(g, w, "%s[%d]" % (path, q))]
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    same = g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes()
    return [] if same else [path or "value"]


def assert_same_bits(got, want, what):
    diff = bits_differ(got, want)
    assert not diff, "%s: not the bits of the private-stream run: %s" % (what, ", ".join(diff))


# ------------------------------------------------------------------------------------------------------ the plain fit
def problem(sa, ora, m, n, k, inv_density=20):
    def make():
        A = ora.synth_csc(m, n, inv_density)
        return A, to_dgc(sa, A), ora.synth_winit(k, m)
    return cached(("problem", m, n, k, inv_density), make)


def run_loop(c, mode, iters):
    from singlet_amd.sharded import nmf_loop
    if mode == "loop":
        return nmf_loop(c, 0.0, iters, L1, L1, 0.0, 0.0)[1]
    if mode == "iterate":
        return np.array([c.nmf_iterate(L1, L1, 0.0, 0.0) for _ in range(iters)])
    it, tols = c.nmf_run(0.0, iters, L1, L1, 0.0, 0.0)
    assert it == iters
    return tols


def plain_fit(c, dA, k, w0, mode, iters=4, upload=True):
    if upload:
        c.upload(dA, None)
    c.fit_init(k, w0)
    tols = run_loop(c, mode, iters)
    W, d, H = c.get_factors()
    return dict(W=W, d=d, H=H, tol=tols)


def private_fit(sa, ora, m, n, k, mode, iters=4):
    def make():
        _, dA, w0 = problem(sa, ora, m, n, k)
        with contexts(sa) as c:
            return plain_fit(c, dA, k, w0, mode, iters)
    return cached(("private", m, n, k, mode, iters), make)


def oracle_fit(sa, ora, m, n, k, iters=4):
    def make():
        A, _, w0 = problem(sa, ora, m, n, k)
        return ora.c_nmf(A, A.t(), 0.0, iters, L1, L1, 0.0, 0.0, 0, w0)
    return cached(("oracle", m, n, k, iters), make)


def assert_at_parity(got, ref, what):
    for key, r in (("W", ref["w"]), ("d", ref["d"]), ("H", ref["h"])):
        err = rel_fro(got[key], r)
        assert err < TOL, "%s: %s is %.3e from the oracle" % (what, key, err)
        assert same_zero_pattern(got[key], r), "%s: zero pattern of %s" % (what, key)


def test_the_stall_outlasts_an_asynchronous_call(sa, ora):
    """The validity of every other test here: a stalled stream is still busy when step_begin, one device-to-device
    hipMemcpyAsync, has returned -- the call was enqueued behind the spin and did not wait for it."""
    _, dA, w0 = problem(sa, ora, 300, 1000, 8)
    with contexts(sa) as c:
        c.upload(dA, None)
        c.fit_init(8, w0)
        run_loop(c, "loop", 1)                             # nothing left to allocate or build
        with caller_stream(c) as S:
            S.synchronize()
            assert S.query()
            the_stall()(S)
            c.step_begin()
            assert not S.query(), "step_begin returned after the stall had ended: STALL_MS is too short, or the call waited"
            S.synchronize()


@pytest.mark.parametrize("upload_first", [True, False], ids=["uploaded_before_set_stream", "uploaded_on_the_stream"])
@pytest.mark.parametrize("k", [8, 50, 100, 136])
def test_plain_fit_on_a_stalled_caller_stream(sa, ora, k, upload_first):
    """k = 8: the generated lane solve; 50: the LDS Gram path; 100: the two-lane solve; 136: the 129 - 256 Gram and the
    four-lane solve.  Through the step API, sgl_nmf_iterate and sgl_nmf_run, a stall before every call."""
    m, n = 300, 1000
    _, dA, w0 = problem(sa, ora, m, n, k)
    for mode in ("loop", "iterate", "run"):
        with contexts(sa) as c:
            if upload_first:
                c.upload(dA, None)
            with caller_stream(c) as S:
                got = plain_fit(Stalled(c, S), dA, k, w0, mode, upload=not upload_first)
        what = "k = %d, %s" % (k, mode)
        assert_same_bits(got, private_fit(sa, ora, m, n, k, mode), what)
        assert_at_parity(got, oracle_fit(sa, ora, m, n, k), what)


@pytest.mark.parametrize("mode", ["loop", "run"])
def test_packed_h_solve_on_a_stalled_caller_stream(sa, mode):
    """70 000 cells: from the second iteration on the H-side solve takes its columns in the order of their previous sweep
    counts (the shape of test_nnls_packing_by_sweep_counts_is_bit_identical); the counters and the order live on the device.
    Compared are the factors, the tol trace and the sweep totals of the columns, as there.  The sweeps per WAVE are not
    a reproducible number: inside one key the counting sort places the columns in the order its LDS atomics give them
    (kernels_nnls.hip), so which columns share a wave differs from run to run on any stream (here: 254 784 against 254 788
    with every other figure the same bits)."""
    def fit(c):
        c.synth(1500, 70000, 20)
        c.fit_init(24, None)
        c.sweeps_get(reset=True)
        tols = run_loop(c, mode, 3)
        sw = c.sweeps_get(reset=True)
        return dict(factors=c.get_factors(), tol=tols, sweeps=dict(h_sweeps=sw["h_sweeps"], w_sweeps=sw["w_sweeps"]))

    def private():
        with contexts(sa) as c:
            return fit(c)
    with contexts(sa) as c, caller_stream(c) as S:
        got = fit(Stalled(c, S))
    want = cached(("packed", mode), private)
    assert want["sweeps"]["h_sweeps"] > 0 and want["sweeps"]["w_sweeps"] > 0
    assert_same_bits(got, want, "packed solve, " + mode)


def test_masked_fit_on_a_stalled_caller_stream(sa, ora):
    """sgl_ard_run, a trace entry every iteration; the oracle at the bar of test_gpu_nmf.py::test_c_ard_nmf_parity."""
    m, n, k, maxit = 200, 600, 10, 4
    A, dA, w0 = problem(sa, ora, m, n, k, 10)

    def fit(c):
        c.upload(dA, None)
        c.fit_init(k, w0)
        tr = c.ard_run(0.0, maxit, L1, 0.0, 77, 20, 1e-3, 1)
        W, d, H = c.get_factors()
        return dict(tr, W=W, d=d, H=H)

    def private():
        with contexts(sa) as c:
            return fit(c)
    with contexts(sa) as c, caller_stream(c) as S:
        got = fit(Stalled(c, S))
    assert_same_bits(got, cached("masked", private), "ard_run")
    ref = ora.c_ard_nmf(A, A.t(), 0.0, maxit, L1, 0.0, 0, w0, 77, 20, 1e-3, 1)
    assert_at_parity(got, ref, "ard_run")
    assert np.array_equal(got["iter"], ref["iter"])
    assert np.allclose(got["test_mse"], ref["test_mse"], rtol=1e-9, atol=0)
    assert np.allclose(got["tol"], ref["tol"], rtol=1e-7, atol=0)


# -------------------------------------------------------------------------------------------------- switching streams
@pytest.mark.parametrize("timing", [False, True], ids=["untimed", "timed"])
def test_switching_streams_mid_fit_keeps_the_bits(sa, ora, timing):
    """2 iterations on the private stream, 2 on S, 2 back on the private stream = 6 on the private stream; with the phase
    timers on (their events are recorded on whichever stream is current and drained at every switch) as well."""
    m, n, k = 300, 1000, 8
    _, dA, w0 = problem(sa, ora, m, n, k)
    want = private_fit(sa, ora, m, n, k, "loop", 6)
    with contexts(sa) as c:
        c.upload(dA, None)
        c.fit_init(k, w0)
        if timing:
            c.timing_enable(True)
        tols = [run_loop(c, "loop", 2)]
        with caller_stream(c) as S:
            tols.append(run_loop(Stalled(c, S), "loop", 2))
        tols.append(run_loop(c, "loop", 2))
        W, d, H = c.get_factors()
        times = c.timing_get() if timing else None
    assert_same_bits(dict(W=W, d=d, H=H, tol=np.concatenate(tols)), want, "private, S, private")
    if timing:
        for phase in ("gram", "rhs_h", "nnls_h", "rhs_w", "nnls_w", "scale"):
            ms, calls = times[phase]
            assert calls >= 6 and ms > 0.0 and np.isfinite(ms), (phase, times[phase])


def test_two_contexts_interleaved_on_one_stream_equal_their_solo_runs(sa, ora):
    shapes = ((300, 1000, 8), (257, 700, 30))
    with contexts(sa, 2) as cs:
        for c, (m, n, k) in zip(cs, shapes):
            _, dA, w0 = problem(sa, ora, m, n, k)
            c.upload(dA, None)
            c.fit_init(k, w0)
        tols = ([], [])
        with caller_stream(*cs) as S:
            for _ in range(4):
                for call, args in STEP_CALLS:
                    for q, c in enumerate(cs):
                        r = getattr(Stalled(c, S), call)(*args)
                        if call == "step_scale_w":
                            tols[q].append(r)
        got = []
        for q, c in enumerate(cs):
            W, d, H = c.get_factors()
            got.append(dict(W=W, d=d, H=H, tol=np.array(tols[q])))
    for g, (m, n, k) in zip(got, shapes):
        assert_same_bits(g, private_fit(sa, ora, m, n, k, "loop"), "interleaved, k = %d" % k)


def test_close_after_a_stalled_asynchronous_step_leaves_the_stream_usable(sa, ora):
    import torch
    _, dA, w0 = problem(sa, ora, 300, 1000, 8)
    with contexts(sa) as c:
        c.upload(dA, None)
        c.fit_init(8, w0)
        with caller_stream(c) as S:
            sc = Stalled(c, S)
            sc.step_begin()
            sc.step_h(L1, 0.0)
            c.close()                                      # with the step still queued behind the stall
            t = torch.arange(1000, dtype=torch.float64, device="cuda:%d" % DEV)   # on S: torch's current stream
            total = float((t * 2.0).sum().item())
            assert S.query()
    assert total == 999000.0


# ------------------------------------------------------------------------------------------ the hook: mirrored shards
class HostDoubler:
    """The all-reduce of two identical shards through the host, with synchronous copies (as PipeSum of
    test_gpu_sharded.py moves its buffers): finished when it returns, whatever stream the context is on."""

    def __init__(self):
        self.hip = ctypes.CDLL("libamdhip64.so")
        self.hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        self.calls = 0

    def __call__(self, ptr, count):
        buf = np.empty(count)
        assert self.hip.hipMemcpy(buf.ctypes.data, ptr, 8 * count, 2) == 0      # device -> host
        buf *= 2.0
        assert self.hip.hipMemcpy(ptr, buf.ctypes.data, 8 * count, 1) == 0      # host -> device
        self.calls += 1


class FakeDist:
    """Stands in for torch.distributed in torch_allreduce_hook: all_reduce over two identical shards = times two, enqueued
    on torch's current stream as a collective would be; `before` runs first (the default-stream test stalls there)."""

    def __init__(self, before=None):
        self.before, self.calls = before, 0

    def all_reduce(self, t, group=None):
        if self.before is not None:
            self.before()
        t.mul_(2.0)
        self.calls += 1


def side_by_side(ora, A):
    """[A | A]"""
    return ora.CSC(np.concatenate([A.x, A.x]), np.concatenate([A.i, A.i]),
                   np.concatenate([A.p, A.p[1:] + A.p[-1]]).astype(A.p.dtype), A.nrow, 2 * A.ncol)


def mirrored_fit(c, dA, k, w0, hook, iters=4):
    c.upload(dA, None, cell_offset=0, ncells_total=2 * dA.ncol)
    c.set_allreduce(hook)
    return plain_fit(c, dA, k, w0, "loop", iters, upload=False)


def host_hook_fit(sa, ora, m, n, k):
    """The mirrored fit on the private stream with the host hook: the reference of both device-hook tests."""
    def make():
        _, dA, w0 = problem(sa, ora, m, n, k)
        hook = HostDoubler()
        with contexts(sa) as c:
            got = mirrored_fit(c, dA, k, w0, hook)
        assert hook.calls >= 8                             # row sums and right-hand sides + Gram, every iteration
        return got
    return cached(("host hook", m, n, k), make)


@pytest.mark.parametrize("m,n,k", [(300, 1000, 8), (257, 700, 30)])
def test_device_hook_on_a_stalled_caller_stream(sa, ora, m, n, k):
    """torch_allreduce_hook on S, the library and the hook enqueueing on the same stalled stream with no host
    synchronisation in between: a host read of the un-reduced buffer, or a kernel off S, would show."""
    import torch
    from singlet_amd.sharded import torch_allreduce_hook
    A, dA, w0 = problem(sa, ora, m, n, k)
    dist = FakeDist()
    with contexts(sa) as c, caller_stream(c) as S:
        got = mirrored_fit(Stalled(c, S), dA, k, w0, torch_allreduce_hook(dist, torch.device("cuda", DEV)))
    assert dist.calls >= 8
    assert_same_bits(got, host_hook_fit(sa, ora, m, n, k), "device hook on S")
    AA = side_by_side(ora, A)
    ref = cached(("oracle AA", m, n, k), lambda: ora.c_nmf(AA, AA.t(), 0.0, 4, L1, L1, 0.0, 0.0, 0, w0))
    assert np.array_equal(ref["h"][:n], ref["h"][n:])
    assert rel_fro(got["W"], ref["w"]) < TOL and rel_fro(got["d"], ref["d"]) < TOL and rel_fro(got["H"], ref["h"][:n]) < TOL


def test_weight_by_split_with_the_device_hook_on_a_stalled_caller_stream(sa, ora):
    import torch
    from singlet_amd.sharded import torch_allreduce_hook
    m, n = 200, 500
    A, dA, _ = problem(sa, ora, m, n, 1, 10)
    sb = np.random.default_rng(9).integers(0, 3, n).astype(np.int32)

    def run(c, hook):
        c.upload(dA, None, cell_offset=0, ncells_total=2 * n)
        c.set_allreduce(hook)
        c.weight_by_split(sb, 3)
        return c.download(0), c.download(1)
    with contexts(sa) as c:
        want = run(c, HostDoubler())
    dist = FakeDist()
    with contexts(sa) as c, caller_stream(c) as S:
        got = run(Stalled(c, S), torch_allreduce_hook(dist, torch.device("cuda", DEV)))
    assert dist.calls >= 1
    assert_same_bits(got, want, "weight_by_split")
    ref = ora.weight_by_split(side_by_side(ora, A), np.concatenate([sb, sb]), 3)
    assert rel_fro(got[0][0], ref.x[:A.x.shape[0]]) < 1e-14


def test_device_hook_with_torch_on_its_default_stream(sa, ora):
    """torch's legacy default stream has handle 0, and set_stream(0) means the context's own, non-blocking stream: the two
    are not ordered against each other.  The private-stream rule then applies to the hook -- finished when it returns --
    so torch_allreduce_hook waits for the default stream itself.  The collective is made slow (a stall in front of it):
    a hook that returns early lets the next kernel read the buffer before it is doubled."""
    import torch
    from singlet_amd.sharded import torch_allreduce_hook
    m, n, k = 300, 1000, 8
    _, dA, w0 = problem(sa, ora, m, n, k)
    stall = the_stall()
    handle = torch.cuda.current_stream(DEV).cuda_stream
    assert handle == 0
    dist = FakeDist(before=lambda: stall(torch.cuda.default_stream(DEV)))
    with contexts(sa) as c:
        c.set_stream(handle)
        got = mirrored_fit(c, dA, k, w0, torch_allreduce_hook(dist, torch.device("cuda", DEV)))
    assert dist.calls >= 8
    assert_same_bits(got, host_hook_fit(sa, ora, m, n, k), "device hook, torch on its default stream")


# ---------------------------------------------------------------------------------------- resident calls after a fit
def resident_calls(m, n, k):
    rng = np.random.default_rng(5)
    labels = (np.arange(n) % 3).astype(np.int32)
    Fm, Fn = rng.random((m, k)), rng.random((n, k))
    G = Fm.T @ Fm + 1e-15 * np.eye(k)
    B = rng.normal(size=(200, k)) * 3 + 1.0
    x, y = rng.random(5000), rng.random(5000)

    def project(c):
        c.project_run(L1, 0.0)
        return c.get_factors()
    return [("evaluate", lambda c: c.evaluate(cell_loss=True, gene_loss=True)),
            ("variable_features", lambda c: c.variable_features(50)),
            ("knn", lambda c: c.knn(10)),
            ("markers", lambda c: c.markers(labels, 3)),
            ("group_means", lambda c: c.group_means(labels, 3)),
            ("project_run", project),
            ("op_gram", lambda c: c.op_gram(Fn)),
            ("op_scale", lambda c: c.op_scale(Fn)),
            ("op_cor", lambda c: c.op_cor(x, y)),
            ("op_rhs 0", lambda c: c.op_rhs(0, Fm)),
            ("op_rhs 1", lambda c: c.op_rhs(1, Fn)),
            ("op_nnls", lambda c: c.op_nnls(G, B, np.zeros_like(B), L1, 0.0)),
            ("op_mse_test", lambda c: c.op_mse_test(77, 20))]


def test_resident_calls_after_a_fit_on_a_stalled_caller_stream(sa, ora):
    m, n, k = 300, 1000, 8
    _, dA, w0 = problem(sa, ora, m, n, k)
    table = resident_calls(m, n, k)

    with contexts(sa) as c:
        plain_fit(c, dA, k, w0, "loop")
        want = {name: call(c) for name, call in table}
    with contexts(sa) as c:
        plain_fit(c, dA, k, w0, "loop")
        with caller_stream(c) as S:
            got = {name: call(Stalled(c, S)) for name, call in table}
    wrong = [name for name, _ in table if bits_differ(got[name], want[name])]
    assert not wrong, "not the bits of the private-stream run: %s" % ", ".join(wrong)


def test_matrix_transforms_on_a_stalled_caller_stream(sa, ora):
    m, n = 300, 1000
    _, dA, _ = problem(sa, ora, m, n, 8)
    rng = np.random.default_rng(6)
    sb = rng.integers(0, 3, n).astype(np.int32)
    rows = rng.permutation(m)[:257].astype(np.int32)
    cols = np.concatenate([rng.permutation(n)[:640], [3, 3]]).astype(np.int32)     # any order, duplicates allowed
    steps = [("log_normalize", lambda c: c.log_normalize(10000.0)),
             ("weight_by_split", lambda c: c.weight_by_split(sb, 3)),
             ("subset", lambda c: c.subset(rows, cols)),
             ("rasterize_rowwise", lambda c: c.rasterize_rowwise(10)),
             ("op_transpose", lambda c: c.op_transpose(0))]

    def run(c):
        c.upload(dA, None)
        out = {}
        for name, step in steps:
            step(c)
            out[name] = (c.dims(), c.download(0), c.download(1))
        return out
    with contexts(sa) as c:
        want = run(c)
    with contexts(sa) as c, caller_stream(c) as S:
        got = run(Stalled(c, S))
    assert want["op_transpose"][0][:2] == (25, 642)
    wrong = [name for name, _ in steps if bits_differ(got[name], want[name])]
    assert not wrong, "not the bits of the private-stream run: %s" % ", ".join(wrong)
