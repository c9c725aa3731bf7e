"""Bit-reproducible synthetic inputs for the HBV parity tests.

Every array is derived from integer hashing (splitmix64) and exactly
representable float arithmetic only, so the golden-fixture generator
(tests/golden/make_golden.py, run once in the authoring container beside the
reference) and the tests (run anywhere, including the GPU box where the
reference does not exist) see the very same bits without the inputs having to
be stored in the fixtures.

Shapes follow the reference's conventions:
  x_phy       [T, B, 3]   forcings ordered (prcp, tmean, pet)
  parameters  [T, B, ny]  raw NN output, column = i_param * nmul + j_member
"""
from __future__ import annotations

import numpy as np

_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _splitmix64(z: np.ndarray) -> np.ndarray:
    z = (z + np.uint64(0x9E3779B97F4A7C15)) & _M64
    z = ((z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & _M64
    z = ((z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & _M64
    return z ^ (z >> np.uint64(31))


def uniform(shape, seed: int, stream: int = 0) -> np.ndarray:
    """U[0,1) with 24 random bits per element (exact in float32)."""
    n = int(np.prod(shape))
    with np.errstate(over="ignore"):
        idx = np.arange(n, dtype=np.uint64)
        key = np.uint64((seed * 0x100000001B3 + stream * 0x9E3779B1 + 0x1234567) & 0xFFFFFFFFFFFFFFFF)
        bits = _splitmix64(_splitmix64(idx ^ key) + key)
    u = (bits >> np.uint64(40)).astype(np.float64) / float(1 << 24)
    return u.reshape(shape).astype(np.float32)


def normalish(shape, seed: int, stream: int = 0) -> np.ndarray:
    """Approximately N(0,1): Irwin-Hall sum of 4 uniforms, exact arithmetic."""
    acc = np.zeros(shape, dtype=np.float64)
    for k in range(4):
        acc += uniform(shape, seed, stream * 8 + k + 101).astype(np.float64)
    # var of one U is 1/12 -> sum of 4 has var 1/3; scale by sqrt(3) rounded to
    # a short binary fraction so the product stays exact in float64.
    return ((acc - 2.0) * 1.734375).astype(np.float32)


def forcing(T: int, B: int, seed: int, cold: bool = False, day0: float = 0.0) -> np.ndarray:
    """CAMELS-shaped synthetic forcing [T,B,3] (prcp mm/d, tmean degC, pet mm/d).

    ~30 % wet days, temperature with a triangular seasonal cycle that crosses
    the parTT range [-2.5, 2.5] so both rain and snow branches are exercised.
    cold=True forces a cold, dry start (ties: melt = SNOWPACK = 0).  Row t is day `day0` + t of the year (day 0 is
    midwinter, where PET is exactly 0 on half of the days).
    """
    u = uniform((T, B, 3), seed, 1).astype(np.float64)
    day = np.arange(T, dtype=np.float64)[:, None] + day0
    phase = (day % 365.0) / 365.0
    tri = np.where(phase < 0.5, 4.0 * phase - 1.0, 3.0 - 4.0 * phase)  # [-1,1]
    boff = uniform((1, B), seed, 2).astype(np.float64) * 20.0 - 8.0
    P = np.maximum(0.0, (u[:, :, 0] - 0.7) * 60.0)
    Tm = 12.0 * tri + (u[:, :, 1] * 14.0 - 7.0) + boff
    PET = np.maximum(0.0, 2.5 + 2.5 * tri + (u[:, :, 2] - 0.5) * 2.0)
    if cold:
        n = min(T, 12)
        P[:n] = 0.0
        Tm[:n] = -15.0 - u[:n, :, 1]
        PET[: n // 2] = 0.0
    return np.stack([P, Tm, PET], axis=-1).astype(np.float32)


def raw_parameters(T: int, B: int, ny: int, seed: int, scale: float = 1.0) -> np.ndarray:
    """Raw (pre-sigmoid) NN output [T,B,ny]."""
    return (normalish((T, B, ny), seed, 3) * np.float32(scale)).astype(np.float32)


def unit_parameters(shape, seed: int, stream: int = 4) -> np.ndarray:
    """Parameters already in (0,1) (Hbv_2 tuple form, no sigmoid)."""
    return (uniform(shape, seed, stream) * np.float32(0.96) + np.float32(0.02)).astype(np.float32)


def loss_weights(shape, seed: int, stream: int = 5) -> np.ndarray:
    return normalish(shape, seed, stream)


def _tri(phase: np.ndarray) -> np.ndarray:
    """Triangular wave on phase in [0,1): -1 at 0, +1 at 0.5."""
    return np.where(phase < 0.5, 4.0 * phase - 1.0, 3.0 - 4.0 * phase)


def forcing_hourly(T: int, B: int, seed: int, storm: float = 4.0, day0: float = 0.0) -> np.ndarray:
    """Hourly synthetic forcing [T,B,3] (prcp mm/h, tmean degC, pet mm/h) for the sub-daily model.

    The season and a diurnal cycle advance with t / 24 (row t is hour t of day `day0` + t / 24; day 0 is midwinter), so
    a record of 8760 rows is one water year: snow accumulates, then melts out.  ~12 % wet hours of up to 3 mm/h, and in
    ~4 % of the 6-hour blocks of a basin a storm burst of `storm` x that (up to 12 mm/h at the default: above the
    infiltration capacity of a wet soil with a small parFMIN * parF0).  PET follows the season and the hour of the day
    (a small residual at night, never an exact zero in summer).  Same exact-arithmetic recipe as `forcing`."""
    u = uniform((T, B, 3), seed, 31).astype(np.float64)
    hour = np.arange(T, dtype=np.float64)[:, None]
    day = day0 + hour / 24.0
    season = _tri((day % 365.0) / 365.0)
    diurnal = _tri(((day0 * 24.0 + hour) % 24.0) / 24.0)         # -1 at midnight, +1 at noon
    boff = uniform((1, B), seed, 32).astype(np.float64) * 20.0 - 8.0
    nblk = (T + 5) // 6
    burst = (uniform((nblk, B), seed, 33).astype(np.float64) < 0.04)
    burst = np.repeat(burst, 6, axis=0)[:T]
    base = np.maximum(0.0, (u[:, :, 0] - 0.88) * 25.0)
    P = np.where(burst, storm * (0.5 + 2.5 * u[:, :, 0]), base)
    Tm = 12.0 * season + 3.0 * diurnal + (u[:, :, 1] * 6.0 - 3.0) + boff
    PET = np.maximum(0.0, 2.5 + 2.5 * season + (u[:, :, 2] - 0.5) * 2.0) * (np.maximum(diurnal, 0.0) / 6.0 + 1.0 / 64.0)
    return np.stack([P, Tm, PET], axis=-1).astype(np.float32)


def wet_states(B: int, M: int, seed: int) -> np.ndarray:
    """Carried-in storages [5,B,M] (SNOWPACK, MELTWATER, SM, SUZ, SLZ; mm) of a wet catchment: a snowpack of up to 40 mm
    on half of the lanes, soil moisture up to and above the range of parFC (50-1000), an upper zone across the range of
    parUZL (0-100), and -- on one lane in eight -- a dry column: soil moisture of 0.0005 mm over a lower zone carried in
    empty (below the model's storage floor; no capillary rise refills that soil)."""
    u = uniform((6, B, M), seed, 34).astype(np.float64)
    SP = np.where(u[0] < 0.5, u[5] * 40.0, 0.0)
    MW = u[1] * 3.0 * (SP > 0)
    dry = u[4] < 0.125
    SM = np.where(dry, 0.0005, u[2] * 1200.0)
    SUZ = u[3] * 150.0
    SLZ = np.where(dry, 0.0, u[4] * 80.0)
    return np.stack([SP, MW, SM, SUZ, SLZ]).astype(np.float32)
