"""Device time of the snap pass and of one sixth-order Hermite step beside the jerk pass and one fourth-order step of the same build, and
what the higher order buys on a Plummer sphere at matched energy error (raw output: profiles/hermite6_measure.txt).

One MI355X, one session, every part a process of its own under a time limit of its own, the parts chained:

    timeout -k 10 300 python tools/hermite6_measure.py passes && timeout -k 10 300 python tools/hermite6_measure.py plummer

passes   N = 65536 (reference box, distinct masses, eps = 0), one fp64 context with time_kernels, three alternating rounds, warmed up:
    jerk f64        nbody_get_jerk_f64: one pass under NBODY_KERNEL_FORCES
    snap f64        nbody_get_snap_f64 with a given acc_in: one pass under NBODY_KERNEL_FORCES
    hermite step    nbody_hermite_step(dt, reps) from a valid cache: one jerk pass and one update (predictor + corrector) per step
    hermite6 step   nbody_hermite6_step(dt, reps) from a valid cache: one snap pass and one update per step
  Device times are nbody_kernel_time's (HIP events around the queued unit).
plummer  N = 4096 (ic_plummer, eps = 0), one frame of 0.05 time units (0.16 crossing times) from the same start: steps, |dE / E| and
  host wall time of nbody_hermite_advance (eta 0.02 and 0.01) and of nbody_hermite6_advance over a ladder of eta, each run twice (the
  second is reported).  "matched" names the largest sixth-order eta whose |dE / E| does not exceed the fourth-order run's."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def passes():
    import parallelnbody_amd as nb
    from parallelnbody_amd import _lib
    F, U = _lib.KERNEL_FORCES, _lib.KERNEL_UPDATE
    n, reps, dt = 65536, 5, 1e-4
    print(f"# passes: fp64 state, theta = 0, N = {n}, eps = 0, dt = {dt}: device ms per call / per step, {reps} repetitions a row")
    posm, vel = nb.ic_reference_box(n, 1000.0, seed=n)
    with nb.NBodyEngine(n, precision="f64", time_kernels=True) as e:
        e.set_state(posm.astype(np.float64), vel.astype(np.float64))
        acc = e.jerk(np.float64)[0]
        e.snap(acc)
        e.synchronize()

        def timed_steps(step):
            step(dt, 2)                                            # warm: this scheme's cache is valid from here on
            e.synchronize()
            e.kernel_time_reset()
            step(dt, reps)
            e.synchronize()
            (f_ms, f_n), (u_ms, u_n) = e.kernel_time(F), e.kernel_time(U)
            assert (f_n, u_n) == (reps, reps), (f_n, u_n)           # one pass and one update per step
            return f_ms / reps, u_ms / reps

        for rnd in range(3):
            e.kernel_time_reset()
            for _ in range(reps):
                e.jerk(np.float64)
            jerk = e.kernel_time(F)[0] / reps
            e.kernel_time_reset()
            for _ in range(reps):
                e.snap(acc)
            ms, count = e.kernel_time(F)
            assert count == reps, count
            snap = ms / reps
            f4, u4 = timed_steps(e.hermite_step)
            f6, u6 = timed_steps(e.hermite6_step)
            print(f"round {rnd}  jerk f64       {jerk:8.4f} ms  {float(n) * n / (jerk * 1e-3):.3e} pairs/s")
            print(f"round {rnd}  snap f64       {snap:8.4f} ms  {float(n) * n / (snap * 1e-3):.3e} pairs/s   snap / jerk {snap / jerk:.4f}")
            print(f"round {rnd}  hermite step   {f4 + u4:8.4f} ms  = forces {f4:8.4f} + update {u4:8.4f}   step / jerk {(f4 + u4) / jerk:.4f}")
            print(f"round {rnd}  hermite6 step  {f6 + u6:8.4f} ms  = forces {f6:8.4f} + update {u6:8.4f}   step / snap {(f6 + u6) / snap:.4f}"
                  f"   hermite6 step / hermite step {(f6 + u6) / (f4 + u4):.4f}")


def plummer():
    import parallelnbody_amd as nb
    n, frame = 4096, 0.05
    print(f"# plummer: fp64 state, N = {n} (ic_plummer, seed 1), eps = 0, one frame of {frame}: steps, |dE / E|, host wall ms (second of two runs)")
    p32, v32 = nb.ic_plummer(n, seed=1)
    posm, vel = p32.astype(np.float64), v32.astype(np.float64)
    rows = []
    with nb.NBodyEngine(n, precision="f64") as e:
        def run(name, advance, eta):
            for _ in range(2):
                e.set_state(posm, vel)
                e0 = sum(e.energy())
                e.synchronize()
                t0 = time.perf_counter()
                t_done, steps = advance(frame, eta=eta, max_steps=200000)
                e.synchronize()
                wall = (time.perf_counter() - t0) * 1e3
                de = abs((sum(e.energy()) - e0) / e0)
            assert t_done == frame, (name, eta, t_done, steps)
            print(f"{name:9s} eta {eta:<6g} steps {steps:6d}  |dE / E| {de:.3e}  wall {wall:9.3f} ms  {wall / steps * 1e3:8.2f} us / step")
            rows.append((name, eta, steps, de, wall))
        for eta in (0.02, 0.01):
            run("hermite", e.hermite_advance, eta)
        for eta in (1.0, 0.8, 0.6, 0.5, 0.4, 0.3, 0.2, 0.15, 0.1):
            run("hermite6", e.hermite6_advance, eta)
    for ref in (r for r in rows if r[0] == "hermite"):
        fit = [r for r in rows if r[0] == "hermite6" and r[3] <= ref[3]]
        if not fit:
            print(f"matched to hermite eta {ref[1]:g}: no sixth-order row reaches |dE / E| {ref[3]:.3e}")
            continue
        m = max(fit, key=lambda r: r[1])
        print(f"matched to hermite eta {ref[1]:g} (|dE / E| {ref[3]:.3e}): hermite6 eta {m[1]:g} (|dE / E| {m[3]:.3e}): "
              f"steps {ref[2]} : {m[2]} = {ref[2] / m[2]:.2f}, wall {ref[4]:.3f} : {m[4]:.3f} ms = {ref[4] / m[4]:.2f}")


if __name__ == "__main__":
    part = sys.argv[1] if len(sys.argv) == 2 else ""
    if part not in ("passes", "plummer"):
        sys.exit(__doc__)
    print(f"# python tools/hermite6_measure.py {part} on one MI355X")
    {"passes": passes, "plummer": plummer}[part]()
