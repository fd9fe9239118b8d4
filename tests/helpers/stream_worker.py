"""Child process of tests/test_streams_gpu.py (part B): the engine on a CALLER's stream, between torch work queued ahead of it and behind
it on that stream with no host wait in between — the ordering parallelnbody_amd/sharded.py rests on.  torch brings its HIP runtime up
first here, as in every ShardedSimulation run.  Prints one `ok: <precision>: <check>` line per check.

Every check queues a delay (torch.cuda._sleep, calibrated to 50 ms and more) on the stream first, records an event behind it, and finds
that event still pending immediately before each engine call: the engine's work is queued while the stream is provably busy.  The twin
of each check is a context of the same parameters on its own stream that is waited for before every call."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import parallelnbody_amd as nb  # noqa: E402

DT, K = 1e-4, 256                                                  # (K passes stay below the timers' drain threshold: no host wait inside a step)
DELAY_MS = 80.0
dev = torch.device("cuda:0")


def delay_cycles():
    """cycles of torch.cuda._sleep that last DELAY_MS, from two events; a loop of large matmuls stands in if the build has no _sleep"""
    if not hasattr(torch.cuda, "_sleep"):
        return None
    cycles = 10_000_000
    for _ in range(8):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(cycles)
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        if ms >= DELAY_MS:
            return cycles
        cycles = int(cycles * min(16.0, 1.25 * DELAY_MS / max(ms, 1e-3))) + 1
    raise AssertionError(f"torch.cuda._sleep({cycles}) lasts {ms} ms: no delay of {DELAY_MS} ms found")


CYCLES = delay_cycles()
_mat = None if CYCLES is not None else torch.randn(4096, 4096, device=dev)


def busy(stream):
    """the delay on `stream`, and the event behind it"""
    with torch.cuda.stream(stream):
        if CYCLES is not None:
            torch.cuda._sleep(CYCLES)
        else:
            x = _mat
            for _ in range(400):
                x = _mat @ x
        ev = torch.cuda.Event()
        ev.record(stream)
    return ev


def scene(n, seed):
    p32, v32 = nb.ic_plummer(n, seed=seed)
    posm, vel = p32.astype(np.float64), v32.astype(np.float64)
    posm[:, :3] += 1e-7 * posm[:, :3] ** 2 + 1e-9
    posm[:, 3] *= 1.0 + 0.5 * np.arange(n) / n
    vel[:, 3] = 0.0
    return posm, vel


def bound(n, precision, own, posm, vel):
    """a time_kernels context whose state lives in torch tensors: (engine, posm_t, vel_t, acc_t)"""
    tdt = torch.float64 if own == np.float64 else torch.float32
    ts = [torch.tensor(x.astype(own), device=dev) for x in (posm, vel)] + [torch.zeros((n, 4), dtype=tdt, device=dev)]
    torch.cuda.synchronize(dev)                                    # (torch filled them on its default stream)
    e = nb.NBodyEngine(n, precision=precision, time_kernels=True)
    e.bind_device_state(*ts)
    return (e, *ts)


def same(a, b, what):
    assert a.tobytes() == b.tobytes(), what


def launches(e):
    return e.kernel_time(nb._lib.KERNEL_FORCES)[1], e.kernel_time(nb._lib.KERNEL_UPDATE)[1]


def run(precision, n):
    own = np.float64 if precision == "f64" else np.float32
    query = (lambda e: e.potentials_f64()) if precision == "f64" else (lambda e: e.potentials())
    posm, vel = scene(n, n)
    new = posm.copy()
    new[:, :3] = scene(n, n + 1)[0][:, :3]                         # other positions, the same masses: what a gather writes
    new_t = torch.tensor(new.astype(own), device=dev)
    torch.cuda.synchronize(dev)
    s, s2 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    assert s.cuda_stream != 0
    e, posm_t, vel_t, acc_t = bound(n, precision, own, posm, vel)
    twin = bound(n, precision, own, posm, vel)[0]
    e.set_stream(s.cuda_stream)
    try:
        # -- torch to engine: torch writes the bound positions on s, the engine reads them with no host wait --
        ev = busy(s)
        with torch.cuda.stream(s):
            posm_t.copy_(new_t, non_blocking=True)
        assert not ev.query(), "the delay was over before compute_forces()"
        e.compute_forces()
        assert not ev.query(), "the delay was over before step()"
        e.step(DT, 3)
        assert not ev.query(), "the delay was over before the query"
        phi = query(e)
        twin.set_state(new.astype(own), vel.astype(own))
        twin.synchronize(); twin.compute_forces()
        twin.synchronize(); twin.step(DT, 3)
        twin.synchronize(); phi_twin = query(twin)
        same(phi, phi_twin, "torch to engine: the query's result")
        for name, x, y in zip(("posm", "vel", "acc"), e.state(own), twin.state(own)):
            same(x, y, "torch to engine: " + name)
        print(f"ok: {precision}: torch to engine", flush=True)

        # -- engine to torch: torch reads what the engine's steps wrote, on s and on a stream that waits for an event on s --
        ev = busy(s)
        assert not ev.query(), "the delay was over before step()"
        e.step(DT, K)
        with torch.cuda.stream(s):
            c1 = posm_t.clone()
            done = torch.cuda.Event()
            done.record(s)
        with torch.cuda.stream(s2):
            s2.wait_event(done)
            c2 = posm_t.clone()
        torch.cuda.synchronize(dev)
        p = e.state(own)[0]
        same(c1.cpu().numpy(), p, "engine to torch: the clone on the engine's stream")
        same(c2.cpu().numpy(), p, "engine to torch: the clone on a stream that waited for the engine's")
        twin.synchronize(); twin.step(DT, K)
        same(p, twin.state(own)[0], "engine to torch: the twin")
        print(f"ok: {precision}: engine to torch", flush=True)

        # -- switching back: nbody_set_stream waits for the stream it leaves --
        ev = busy(s)
        assert not ev.query(), "the delay was over before step()"
        e.step(DT, K)
        e.set_stream(None)
        e.step(DT, 3)
        twin.synchronize(); twin.step(DT, K)
        twin.synchronize(); twin.step(DT, 3)
        for name, x, y in zip(("posm", "vel", "acc"), e.state(own), twin.state(own)):
            same(x, y, "switching back: " + name)
        e.set_stream(s.cuda_stream)
        print(f"ok: {precision}: switching back", flush=True)

        # -- timers: the same passes were counted on the caller's stream as on the context's own --
        got, want = launches(e), launches(twin)
        assert got == want and got[0] >= 2 * K + 7, (got, want)
        print(f"ok: {precision}: timers", flush=True)
    finally:
        e.close(); twin.close()


run("f32", 2000)
run("f64", 1025)
