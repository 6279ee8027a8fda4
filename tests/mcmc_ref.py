"""Float64 numpy restatement of the 3DGS-MCMC strategy (include/r3dgs_mcmc.h, reduced-3dgs_amd/r3dgs_mcmc.py), written from
the method's formulas and not from the kernels: the yardstick of csrc/mcmc.hip and csrc/mcmc_math.h.  Shared by
tests/test_mcmc_cpu.py and tests/test_mcmc_gpu.py.

  noise     o = sigmoid(opacity_raw);  gate = 1 / (1 + exp(-100 ((1 - o) - 0.995)));  S = R(q) diag(exp(scaling_raw))^2 R(q)^T,
            q the normalised rotation_raw;  xyz += scale * gate * (S @ noise_row)
  plan      w = sigmoid(opacity_raw), 0 for a dead row (RELOCATE: w <= min_opacity);  cdf = cumsum(w);  draw k = the first j
            with cdf[j] > u_k * cdf[-1];  ratio = 1 + bincount(sampled), clamped to 51;  slots = the dead rows in index order
  relocate  o' = 1 - (1 - o)^(1/N);  D = sum_{i=1..N} sum_{k=0..i-1} C(i-1,k) (-1)^k o'^(k+1) / sqrt(k+1);  s' = (o / D) s;
            o' <- clamp(o', min_opacity, 1 - 2^-23);  opacity_raw = log(o' / (1 - o')), scaling_raw = log(s')
  move      RELOCATE: every drawn source (ratio >= 2) takes its new opacity and scaling, then row slots[k] becomes a copy of
            row sampled[k] (all six parameters and _degrees); both moments are zeroed at the drawn sources and, with
            zero_relocated, at the relocated rows.  GROW: the old rows with the drawn sources updated, then row P + k = a copy
            of the updated row sampled[k]; moments: old rows kept, new rows zero.

Bound of the updated rows (the fp32 evaluation of csrc/mcmc_math.h against this float64 one).  u = U = 2^-24.  The kernel's
o = stats_sigmoid(raw) is within SIGMOID_REL of sigma = sigmoid(raw) (tests/trainstats_ref.py); o' and D are evaluated in
double from it (their own error, ~1e-15, is covered by the 1e-12 added at the end) and rounded to fp32 once.
  kappa = d ln o' / d ln o = o (1 - o)^(1/N - 1) / (N o')          eta = d ln D / d ln o' = o' D'(o') / D
  opacity  L = log(o' / (1 - o')), dL/do' = 1 / (o' (1 - o')).  o' carries SIGMOID_REL kappa + u (its rounding) relative, i.e.
           (SIGMOID_REL kappa + u) / (1 - o') on L (the clamp is 1-Lipschitz and the same on both sides); 1 - o': u; the divide:
           u; logf: LOGF_REL |L|.
  scaling  L = log(o / D) + raw.  o / D carries SIGMOID_REL (1 + |eta kappa|) + u (its rounding); expf(raw): EXPF_REL; the
           product: u; logf: LOGF_REL |L|.
Both are multiplied by 1 + 2^-10 for the second-order terms.  kappa grows like 1 / (1 - o): the tests keep sigmoid(opacity) <=
0.99 so that the bound stays a few hundred u.
"""
import math

import numpy as np

from tests.densify_ref import LOGF_REL
from tests.trainstats_ref import EXPF_REL, SIGMOID_REL, U, sigmoid64

F32 = np.float32
NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
RELOCATE, GROW = 0, 1
MAX_RATIO = 51
MAX_OPACITY = 1.0 - 2.0 ** -23
GATE_STEEP, GATE_CENTRE = 100.0, 0.995
BINOM = np.array([[float(math.comb(n, k)) for k in range(MAX_RATIO)] for n in range(MAX_RATIO)])


# ---- noise -----------------------------------------------------------------------------------------------------------------

def gate(o):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-GATE_STEEP * ((1.0 - np.asarray(o, np.float64)) - GATE_CENTRE)))


def rotation(raw_q):
    """build_rotation of the normalised quaternion (r, x, y, z) -> [n,3,3]."""
    x = np.asarray(raw_q, np.float64)
    q = x / np.maximum(np.sqrt((x * x).sum(axis=1)), 1e-12)[:, None]
    r, qx, qy, qz = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return np.stack([np.stack([1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - r * qz), 2 * (qx * qz + r * qy)], 1),
                     np.stack([2 * (qx * qy + r * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - r * qx)], 1),
                     np.stack([2 * (qx * qz - r * qy), 2 * (qy * qz + r * qx), 1 - 2 * (qx * qx + qy * qy)], 1)], 1)


def covariance(raw_q, raw_scale):
    R = rotation(raw_q)
    s2 = np.exp(np.asarray(raw_scale, np.float64)) ** 2
    return np.einsum("nij,nj,nkj->nik", R, s2, R)


def noise_delta(opacity_raw, scaling_raw, rotation_raw, noise, scale):
    """-> the displacement [P,3] the noise call adds to xyz."""
    g = gate(sigmoid64(np.asarray(opacity_raw).reshape(-1)))
    S = covariance(rotation_raw, scaling_raw)
    return np.float64(F32(scale)) * g[:, None] * np.einsum("nij,nj->ni", S, np.asarray(noise, np.float64))


# ---- plan ------------------------------------------------------------------------------------------------------------------

def weights(opacity_raw, min_opacity, mode):
    """-> (w float64 [P], dead bool [P])."""
    w = sigmoid64(np.asarray(opacity_raw).reshape(-1))
    dead = (w <= np.float64(F32(min_opacity))) if mode == RELOCATE else np.zeros(w.shape, bool)
    return np.where(dead, 0.0, w), dead


def in_band(opacity_raw, min_opacity):
    """bool [P]: sigmoid(raw) is so close to min_opacity that an fp32 sigmoid may decide `dead` differently."""
    w = sigmoid64(np.asarray(opacity_raw).reshape(-1))
    t = np.float64(F32(min_opacity))
    return np.abs(w - t) <= SIGMOID_REL * abs(t)


def keep_out_of_band(opacity_raw, min_opacity):
    for _ in range(8):
        bad = in_band(opacity_raw, min_opacity)
        if not bad.any():
            break
        opacity_raw.reshape(-1)[bad] += F32(2.0 ** -10)
    return opacity_raw


def draws(w, uniforms):
    """-> sampled int [n]: the first j with cdf[j] > u * cdf[-1]."""
    cdf = np.cumsum(w)
    return np.searchsorted(cdf, np.asarray(uniforms, np.float64) * cdf[-1], side="right")


def ratio_of(P, sampled):
    count = np.bincount(np.asarray(sampled, np.int64), minlength=P)
    return np.minimum(1 + count, MAX_RATIO).astype(np.int32), count


def plan_totals(w, dead, mode, n_draws, sampled):
    """The eight totals of a plan whose draws came out as `sampled` (None: no draws were made)."""
    pos = int((w > 0).sum())
    want = int(dead.sum()) if mode == RELOCATE else int(n_draws)
    noop = 1 if pos == 0 else (2 if want == 0 else 0)
    n = 0 if noop else want
    if n:
        _, count = ratio_of(len(w), sampled[:n])
        distinct, clamped = int((count > 0).sum()), int((1 + count > MAX_RATIO).sum())
    else:
        distinct = clamped = 0
    return [int(dead.sum()), n, distinct, clamped, noop, pos, 0, 0]


def n_new(P, cap_max, growth=1.05):
    return max(0, min(int(cap_max), int(growth * P)) - P)


# ---- relocation formula ------------------------------------------------------------------------------------------------------

def relocate_o(o, N):
    return 1.0 - (1.0 - o) ** (1.0 / N)


def relocate_D(o_new, N, derivative=False):
    """The double sum as the method states it (derivative: d/do' of it)."""
    total = 0.0
    for i in range(1, N + 1):
        for k in range(i):
            if derivative:
                total += BINOM[i - 1, k] * (-1) ** k * (k + 1) * o_new ** k / math.sqrt(k + 1)
            else:
                total += BINOM[i - 1, k] * (-1) ** k * o_new ** (k + 1) / math.sqrt(k + 1)
    return total


def relocate_row(raw_opacity, raw_scale, N, min_opacity):
    """One drawn source -> (opacity_raw', scaling_raw' [3], bound of the first, bound of the second [3])."""
    o = float(sigmoid64(np.float64(raw_opacity)))
    o_new = -math.expm1(math.log1p(-o) / N)   # 1 - (1 - o)^(1/N) without the cancellation
    D = relocate_D(o_new, N)
    oc = min(max(o_new, float(F32(min_opacity))), MAX_OPACITY)
    L_op = math.log(oc / (1.0 - oc))
    raw_scale = np.asarray(raw_scale, np.float64)
    L_sc = math.log(o / D) + raw_scale
    kappa = o * (1.0 - o) ** (1.0 / N - 1.0) / (N * o_new)
    eta = o_new * relocate_D(o_new, N, derivative=True) / D
    second = 1.0 + 2.0 ** -10
    b_op = ((SIGMOID_REL * kappa + U) / (1.0 - oc) + 2 * U + LOGF_REL * abs(L_op)) * second + 1e-12
    b_sc = (SIGMOID_REL * (1.0 + abs(eta * kappa)) + 2 * U + EXPF_REL + LOGF_REL * np.abs(L_sc)) * second + 1e-12
    return L_op, L_sc, b_op, b_sc


def updated_rows(opacity_raw, scaling_raw, ratio, min_opacity):
    """-> {i: (opacity', scaling' [3], bound, bound [3])} for every drawn source (ratio >= 2)."""
    op = np.asarray(opacity_raw).reshape(-1)
    return {int(i): relocate_row(op[i], scaling_raw[i], int(ratio[i]), min_opacity) for i in np.flatnonzero(np.asarray(ratio) >= 2)}


# ---- move ------------------------------------------------------------------------------------------------------------------

def _copy_state(state):
    out = {k: (v.copy() if isinstance(v, np.ndarray) else {n: a.copy() for n, a in v.items()}) for k, v in state.items()}
    return out


def relocate(state, sampled, slots, ratio, min_opacity, zero_relocated):
    """state: the six parameters under NAMES, "degrees", optionally "exp_avg" / "exp_avg_sq" dicts by name.  sampled, slots:
    the n_draws draws and their destinations.  -> (new state, updated): the float32 opacity / scaling of the rows in `updated`
    are placeholders -- those rows are compared through the float64 values and bounds there."""
    out = _copy_state(state)
    upd = updated_rows(state["opacity"], state["scaling"], ratio, min_opacity)
    for i, (op, sc, _, _) in upd.items():
        out["opacity"][i] = F32(op)
        out["scaling"][i] = sc.astype(F32)
    drawn = np.asarray(ratio) >= 2
    sampled, slots = np.asarray(sampled, np.int64), np.asarray(slots, np.int64)
    for name in NAMES + ("degrees",):
        out[name][slots] = out[name][sampled]
    for key in ("exp_avg", "exp_avg_sq"):
        if key in out:
            for name in out[key]:
                out[key][name][drawn] = 0
                if zero_relocated:
                    out[key][name][slots] = 0
    return out, upd


def grow(state, sampled, ratio, min_opacity):
    """-> (new state of P + len(sampled) rows, updated)."""
    sampled = np.asarray(sampled, np.int64)
    base, upd = relocate(state, [], [], ratio, min_opacity, False)
    for key in ("exp_avg", "exp_avg_sq"):   # growth keeps the old rows' moments, the drawn sources' too
        if key in state:
            base[key] = {n: a.copy() for n, a in state[key].items()}
    out = {}
    for name in NAMES + ("degrees",):
        out[name] = np.concatenate([base[name], base[name][sampled]], axis=0)
    for key in ("exp_avg", "exp_avg_sq"):
        if key in base:
            out[key] = {n: np.concatenate([a, np.zeros((len(sampled),) + a.shape[1:], a.dtype)], axis=0) for n, a in base[key].items()}
    return out, upd
