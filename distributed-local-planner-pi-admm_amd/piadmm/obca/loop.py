"""The loop (csrc/piadmm_obca_plan_loop.hip, piadmm_obca_loop_plan): the closed loop of a clocked plan --
plant, noise and delay at the step index k0 + c of each tenant's own clock -- in NumPy."""
import numpy as np

from .._lib import FEEDBACK_PAR
from .feedback import (NOISE_K_MAX, delay_args, delay_tau, feedback_row, feedback_row_check, noise_args, noise_tape)
from .model import NX


# the loop items of piadmm_obca_plan_get: name -> (code, dtype) (PIADMM_OBCA_LOOP_GET_*)
LOOP_GET = {"LOOP_PLANT": (43, np.float64), "LOOP_NOISE": (44, np.float64), "LOOP_DELAY": (45, np.float64),
            "LOOP_TAU": (46, np.float64), "LOOP_STREAMS": (47, np.int64), "LOOP_SEED": (48, np.uint64)}
# the loop's flags (the tenant header's word 11, LOOP_SEED[2])
LOOP_ON, LOOP_NOISE, LOOP_DELAY = 1, 2, 4


def loop_args(n, plant=None, noise=None, delay=None, streams=None, seed=0, k0=0):
    """dict(plant, noise, delay, streams, seed, k0) of a planner's loop argument, checked as
    piadmm_obca_loop_plan checks it: plant one plant row or n (None: the nominal row), noise one noise
    row or n (None: no noise), delay one delay row or n (None: no delay), each as rows x its width;
    streams n int64 >= 0 (None: 0 .. n-1), seed a uint64, 0 <= k0 < 2^31."""
    plant = feedback_row() if plant is None else plant
    plant = np.ascontiguousarray(np.asarray(plant, np.float64).reshape(-1, FEEDBACK_PAR))
    if plant.shape[0] not in (1, n):
        raise ValueError(f"obca.loop: plant rows must be 1 or n ({n})")
    for k, row in enumerate(plant):
        why = feedback_row_check(row)
        if why is not None:
            raise ValueError(f"obca.loop: plant row {k}: {why}")
    # the streams, the seed and k0 through the one statement of them
    _, streams, seed, k0 = noise_args(n, None, streams, seed, k0)
    if noise is not None:
        noise = noise_args(n, noise, streams, seed, k0)[0]
    if delay is not None:
        delay = delay_args(n, delay, streams, seed, k0)[0]
    return dict(plant=plant, noise=noise, delay=delay, streams=streams, seed=seed, k0=k0)


def loop_draw(n, clock, noise=None, delay=None, streams=None, seed=0, k0=0):
    """(w, tau) of piadmm_obca_loop_draw, host restatement: w[s] (n x 2 x 5) the disturbance row and
    tau[s] (n x 2) the latency of stream streams[s] (None: s) at step index k0 + clock[s][0] -- row
    [s][c_s] of `noise_tape` / `delay_tau` -- under noise / delay (one row or n; None: zeros).  clock
    n x 3 as the CLOCK item (only c is read) or n clocks."""
    n = int(n)
    clock = np.asarray(clock, np.int64)
    c = clock.reshape(n, -1)[:, 0]
    a = loop_args(n, None, noise, delay, streams, seed, k0)
    if (c < 0).any() or (a["k0"] + c >= NOISE_K_MAX).any():
        raise ValueError("obca.loop_draw: c >= 0 and every step index k0 + c below 2^31")
    w, tau = np.zeros((n, 2, NX)), np.zeros((n, 2))
    for s in range(n):
        t, k = a["streams"][s:s + 1], a["k0"] + int(c[s])
        if a["noise"] is not None:
            w[s] = noise_tape(1, 1, a["noise"][s % len(a["noise"])], t, a["seed"], k)[0, 0]
        if a["delay"] is not None:
            tau[s] = delay_tau(1, 1, a["delay"][s % len(a["delay"])], t, a["seed"], k)[0, 0]
    return w, tau
