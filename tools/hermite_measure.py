"""Device time of one fourth-order Hermite step beside one fp64 jerk pass of the same build (raw output:
profiles/hermite_measure.txt).

    python tools/hermite_measure.py

N = 65536 (reference box, distinct masses, eps = 0), one fp64 context with time_kernels, three alternating rounds, everything warmed up:
    jerk f64        nbody_get_jerk_f64: one pass under NBODY_KERNEL_FORCES
    hermite step    nbody_hermite_step(dt, reps) from a valid cache: per step one pass under NBODY_KERNEL_FORCES (the jerk pass on the
                    predicted state) and one under NBODY_KERNEL_UPDATE (predictor + corrector)
Device times are nbody_kernel_time's (HIP events around the queued unit)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import parallelnbody_amd as nb
    from parallelnbody_amd import _lib
    n, reps, dt = 65536, 5, 1e-4
    print("# python tools/hermite_measure.py on one MI355X, one session")
    print(f"# fp64 state, theta = 0, N = {n}, eps = 0, dt = {dt}: device ms per call / per step, {reps} repetitions a row")
    posm, vel = nb.ic_reference_box(n, 1000.0, seed=n)
    with nb.NBodyEngine(n, precision="f64", time_kernels=True) as e:
        e.set_state(posm.astype(np.float64), vel.astype(np.float64))
        e.jerk(np.float64)
        e.hermite_step(dt, 2)                                      # warm: the cache is valid from here on
        e.synchronize()
        for rnd in range(3):
            e.kernel_time_reset()
            for _ in range(reps):
                e.jerk(np.float64)
            jerk = e.kernel_time(_lib.KERNEL_FORCES)[0] / reps
            e.kernel_time_reset()
            e.hermite_step(dt, reps)
            e.synchronize()
            (f_ms, f_n), (u_ms, u_n) = e.kernel_time(_lib.KERNEL_FORCES), e.kernel_time(_lib.KERNEL_UPDATE)
            assert (f_n, u_n) == (reps, reps), (f_n, u_n)           # one jerk pass and one update per step
            forces, update = f_ms / reps, u_ms / reps
            print(f"round {rnd}  jerk f64      {jerk:8.4f} ms  {float(n) * n / (jerk * 1e-3):.3e} /s")
            print(f"round {rnd}  hermite step  {forces + update:8.4f} ms  = forces {forces:8.4f} + update {update:8.4f}   "
                  f"step / jerk {(forces + update) / jerk:.4f}")


if __name__ == "__main__":
    main()
