"""First-order (Gauss-Newton / Laplace) uncertainty of a per-basin calibration.

`normal_equations` already holds what a first-order answer needs: JtJ is the information matrix of every basin, and
its inverse scaled by the residual variance is the parameter covariance Sigma_b (`parameter_covariance`).  The part of
the variance of a simulated series that comes from the parameters is then
    var[t,b] = s[:,t,b]^T Sigma_b s[:,t,b],
s[:,t,b] the Jacobian row of that basin-day.  `predictive_variance` forms it straight from the direction-major series
the tangent kernels write ([C,T_out,B], the basin as the unit-stride axis) with one hbvx_quadform call
(include/hbvx.h): the permuted Jacobian [T_out,B,C] and its product with Sigma, two more arrays of the size of the
series, are never built.  The covariance travels as a lower-triangular factor M_b with M_b^T M_b = Sigma_b, so the
result is |M_b s|^2: half the multiply-adds, and never negative.  With the factor of (JtJ)^-1 the same call gives the
leverage (the diagonal of the hat matrix) over the weight.

Models, keys and refusals are those of `normal_equations`: basins are independent in Hbv, Hbv_1_1p, Hbv_2 and HbvAdj;
Hbv_2_hourly and Hbv_2_mts route to gages, which couple the units: refused.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from . import ops
from ._lib import get_library
from .calibrate import _NO_TARGET, _check_request, _primal_and_series


def _prior(prior_precision, B: int, C: int, device) -> torch.Tensor:
    p = torch.as_tensor(prior_precision, dtype=torch.float64, device=device)
    if p.dim() == 0:
        p = p.expand(B, C)
    elif tuple(p.shape) == (C,):
        p = p.unsqueeze(0).expand(B, C)
    elif tuple(p.shape) != (B, C):
        raise ValueError(f"prior_precision must be a number, [{C}] or [{B},{C}], got {tuple(p.shape)}")
    if not bool(torch.isfinite(p).all()) or bool((p < 0).any()):
        raise ValueError("prior_precision must be finite and must not be negative")
    return p


def parameter_covariance(neq: dict, prior_precision=0.0, sigma2=None, eps: float = 1e-12) -> dict:
    """Per-basin parameter covariance from a `normal_equations` result, in float64:
        A_b = JtJ_b / sigma2_b + diag(prior_precision),   cov_b = A_b^-1.
    prior_precision   a number, [C] or [B,C], >= 0: the precision (1 / variance) of an independent Gaussian prior on
                      every column, in the space the module takes the parameters in.
    sigma2            the residual variance: a number or [B]; default cost / (n_obs - C), the usual unbiased estimate
                      (it needs neq['cost'] and neq['n_obs']).
    eps               a basin whose smallest squared Cholesky pivot is not above eps times the largest diagonal
                      element of A counts as not positive definite.
    Returns {'cov' [B,C,C], 'std' [B,C], 'corr' [B,C,C] (float64), 'sigma2' [B] (float64), 'factor' [B,C,C] float32
    lower-triangular with factor^T factor = cov (with A = R R^T the Cholesky factorisation, factor = R^-1; what
    `predictive_variance` takes), 'failed' [B] bool, 'columns'}.  A basin is `failed` -- all its outputs are zero --
    when n_obs <= C and no sigma2 was given, when sigma2 is not a positive finite number, when A is not finite, or when
    A is not positive definite (as `lm_step` flags it).  Covariances are in the space the module takes its parameters
    in: raw for Hbv / Hbv_1_1p / HbvAdj, as `calibrate` documents."""
    JtJ = neq['JtJ']
    if JtJ.dim() != 3 or JtJ.shape[1] != JtJ.shape[2]:
        raise ValueError(f"neq['JtJ'] must be [B,C,C], got {tuple(JtJ.shape)}")
    B, C = int(JtJ.shape[0]), int(JtJ.shape[1])
    dev = JtJ.device
    H = JtJ.to(torch.float64)
    prior = _prior(prior_precision, B, C, dev)
    if sigma2 is None:
        dof = neq['n_obs'].to(device=dev, dtype=torch.float64) - C
        short = dof <= 0
        s2 = neq['cost'].to(device=dev, dtype=torch.float64) / torch.where(short, torch.ones_like(dof), dof)
    else:
        s2 = torch.as_tensor(sigma2, dtype=torch.float64, device=dev)
        if s2.dim() == 0:
            s2 = s2.expand(B)
        if tuple(s2.shape) != (B,):
            raise ValueError(f"sigma2 must be a number or [{B}], got {tuple(s2.shape)}")
        short = torch.zeros(B, dtype=torch.bool, device=dev)
    bad = short | ~torch.isfinite(s2) | (s2 <= 0)
    s2 = torch.where(bad, torch.ones_like(s2), s2)
    A = H / s2[:, None, None] + torch.diag_embed(prior)
    bad = bad | ~torch.isfinite(A).all(-1).all(-1)
    eye = torch.eye(C, dtype=torch.float64, device=dev)
    A = torch.where(bad[:, None, None], eye, A)
    R, status = torch.linalg.cholesky_ex(A)
    pivot = torch.diagonal(R, dim1=1, dim2=2).square().amin(-1)
    scale = torch.diagonal(A, dim1=1, dim2=2).amax(-1)
    failed = bad | (status != 0) | ~(pivot > eps * scale)
    R = torch.where(failed[:, None, None], eye, R)
    factor = torch.linalg.solve_triangular(R, eye.expand(B, C, C), upper=False)        # R^-1, lower
    factor = torch.tril(factor)
    cov = factor.transpose(1, 2) @ factor
    std = torch.sqrt(torch.diagonal(cov, dim1=1, dim2=2))
    corr = cov / (std[:, :, None] * std[:, None, :])
    keep = (~failed)[:, None, None]
    zero = torch.zeros_like(cov)
    out = {'cov': torch.where(keep, cov, zero), 'std': torch.where(keep[:, :, 0], std, zero[:, :, 0]),
           'corr': torch.where(keep, corr, zero), 'sigma2': torch.where(failed, torch.zeros_like(s2), s2),
           'factor': torch.where(keep, factor, zero).to(torch.float32), 'failed': failed}
    if 'columns' in neq:
        out['columns'] = list(neq['columns'])
    return out


def covariance_factor(cov: torch.Tensor) -> torch.Tensor:
    """The factor `predictive_variance` takes, for a covariance from elsewhere: M [B,C,C] float32, lower-triangular,
    with M^T M = cov.  Computed in float64 as the Cholesky factor of the index-reversed matrix, reversed back and
    transposed (P cov P = L L^T gives cov = U U^T with U = P L P upper-triangular, and M = U^T).  A covariance that is
    not finite, not symmetric or not positive definite raises ValueError."""
    if not torch.is_tensor(cov) or cov.dim() != 3 or cov.shape[1] != cov.shape[2]:
        raise ValueError(f"cov must be [B,C,C], got {tuple(cov.shape) if torch.is_tensor(cov) else type(cov).__name__}")
    S = cov.to(torch.float64)
    if not bool(torch.isfinite(S).all()):
        raise ValueError("cov holds non-finite values")
    if not torch.allclose(S, S.transpose(1, 2), rtol=1e-6, atol=0.0):
        raise ValueError("cov is not symmetric")
    L, status = torch.linalg.cholesky_ex(torch.flip(S, dims=(1, 2)))
    if bool((status != 0).any()):
        which = torch.nonzero(status != 0).flatten().tolist()
        raise ValueError(f"cov is not positive definite for basins {which[:8]}{' ...' if len(which) > 8 else ''}")
    return torch.tril(torch.flip(L, dims=(1, 2)).transpose(1, 2)).to(torch.float32).contiguous()


def predictive_variance(model, x_dict: dict, parameters, factor, names: Optional[Sequence[str]] = None,
                        key: Optional[str] = None, max_directions: int = 64) -> dict:
    """The parameter part of the first-order variance of one output series:
        {'var': [T_out,B] float32 >= 0, var[t,b] = |factor[b] @ J[t,b,:]|^2 = J[t,b,:] Sigma_b J[t,b,:]^T,
         'outputs': the primal flux dictionary, 'columns': [C indices]}
    with J as `parameter_jacobian` (HbvAdj: `adj_parameter_jacobian`) defines it and Sigma_b = factor[b]^T factor[b].
    model, names, key   as in `normal_equations`.
    factor              [B,C,C], lower-triangular, columns in the order of `columns`: 'factor' of
                        `parameter_covariance`, or `covariance_factor(cov)`.  What lies above the diagonal is ignored.
    x_dict              may be another period than the one calibrated on: that is the point.
    The module runs ONCE; the one-hot directions go through the tangent kernels `max_directions` at a time into a
    single [C,T_out,B] float32 buffer, exactly as in `normal_equations`, and one hbvx_quadform call reduces it.  The
    reduction holds that buffer plus the packed factor (C(C+1)/2 * B floats) and no second array of the buffer's size;
    the whole call peaks at about twice the buffer, because the tangent kernels' outputs of a chunk of directions and
    the primal's tensors are alive while it fills (profiles/r13_predictive_variance.md).  Observation noise is not
    included: add sigma2 for a band around observations.  Results are bit-reproducible and do not depend on
    max_directions.

    Refused before the model runs: what `normal_equations` refuses (NotImplementedError, ValueError, KeyError); a
    factor that is not [B, len(columns), len(columns)] or not finite in its lower triangle (ValueError); a library
    without hbvx_quadform (HbvxError)."""
    req = _check_request(model, x_dict, parameters, _NO_TARGET, names, key, None, max_directions,
                         what="predictive_variance")
    C = len(req.cols)
    if not torch.is_tensor(factor) or tuple(factor.shape) != (req.B, C, C):
        raise ValueError(f"factor must be [{req.B},{C},{C}] (basins, then the columns {names or 'of every static name'}"
                         f" twice), got {tuple(factor.shape) if torch.is_tensor(factor) else type(factor).__name__}")
    if not bool(torch.isfinite(torch.tril(factor)).all()):
        raise ValueError("factor holds non-finite values in its lower triangle")
    get_library().require("hbvx_quadform")
    outputs, sim, series = _primal_and_series(model, req, x_dict, parameters, max_directions)
    fac = factor.to(device=sim.device, dtype=torch.float32)
    return {'var': ops.quadform(series, fac), 'outputs': outputs, 'columns': list(req.cols)}
