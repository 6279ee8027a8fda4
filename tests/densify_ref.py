"""Numpy restatement of the reference's densification (scene/gaussian_model.py:502-522, :553-691) on plain CPU arrays: the
yardstick of reduced-3dgs_amd/r3dgs_densify.py, csrc/densify.hip and csrc/densify_math.h.  Shared by tests/test_densify_cpu.py
and tests/test_densify_gpu.py; tools/densify_bench.py takes its byte count from it.

What the reference's lines do, in the order they run (densify_and_prune, :670-682):

  :671-672  grads = xyz_gradient_accum / denom; grads[isnan] = 0.  0/0 becomes 0; x/0 = inf stays and passes the threshold.
  :651-668  densify_and_clone.  mask = grads >= max_grad and max(exp(_scaling)) <= percent_dense * extent.  The masked rows of
            every parameter and of _degrees are appended as they are (cat_tensors_to_optimizer :570-598: exp_avg and
            exp_avg_sq get zero rows, and .grad with store_grads); densification_postfix (:617-620) replaces
            xyz_gradient_accum, density_gradient_accum, denom and max_radii2D by zeros of the new size.
  :622-649  densify_and_split.  The gradient is padded with ZEROS for the clones just appended (:626-627), so with
            max_grad > 0 no clone is selected; with max_grad <= 0 every clone would be (the entry point refuses that).
            mask = padded grads >= max_grad and max scale > percent_dense * extent.  N = 2 children per masked row, all
            first children and then all second children (repeat(N, 1)):
              xyz_child     = R(q) (noise * scale) + xyz      build_rotation normalises the raw quaternion (:636-637)
              scaling_child = log(scale / (0.8 N))            (:638)
              everything else is the parent's raw row (:639-643)
            They are appended (zero moments), then prune_points drops the parents (:647-648).
  :684-691  prune, on the set after clone and split.  mask = sigmoid(_opacity) < min_opacity; if max_screen_size is truthy
            also max_radii2D > max_screen_size or max(exp(_scaling)) > 0.1 * extent.
            QUIRK, kept: densification_postfix has zeroed max_radii2D by the time densify_and_prune reaches prune, so the
            screen-size term compares 0 with the threshold there; it can act only when prune() is called on its own.
            The children's world-size term looks at exp(scaling_child), the activation of the stored value.
  :553-568  prune_points(mask): every parameter, both moments (and .grad with store_grads, but only for a group that has
            optimizer state, :511-515), _degrees, xyz_gradient_accum, denom and max_radii2D keep the rows with mask False.
            state['step'] is never touched.  density_gradient_accum is not compacted (the reference does not).

Thresholds are Python doubles rounded to float32 once, as torch does when it compares a float32 tensor with a Python scalar.

Resulting order.  Cat appends and boolean indexing is stable, so the result is four segments in source-index order:
  A  originals that are neither split nor pruned      C  surviving first children
  B  surviving clones                                 D  surviving second children
A clone is its source's row, so it has its source's prune mask; both children of a parent share opacity and scaling, so C and
D hold the same parents.  exp_avg / exp_avg_sq (and .grad) rows follow their parameter row in A and are zero in B, C, D.

Decisions are taken here in float64 from the float32 inputs: on inputs that keep out of the ambiguity bands below, any
float32 evaluation within the documented accuracy of expf / logf takes the same ones.
"""
import numpy as np

from tests.trainstats_ref import EXPF_REL, SIGMOID_REL, U, sigmoid64

F32 = np.float32
NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
N_CHILDREN = 2
CHILD_SHRINK = F32(0.8 * N_CHILDREN)   # the Python double 1.6, rounded once where torch divides a float32 tensor by it

# Documented accuracy of logf: 1 ulp on the host (glibc, x86_64) and on the device (HIP math API): at most 2 U relative.
LOGF_REL = 2 * U

# ---- ambiguity bands of the decisions ------------------------------------------------------------------------------------------
# scale = expf(raw) is within EXPF_REL of exp(raw): a float32 evaluation can only disagree with the float64 one about
# `scale <=> t` when exp(raw) lies within EXPF_REL * t of t (second order added).
SCALE_BAND_REL = EXPF_REL + 8 * U * U
# sigmoid(raw) <=> min_opacity: trainstats_ref derives SIGMOID_REL for csrc/stats_math.h's sigmoid.
OPACITY_BAND_REL = SIGMOID_REL


def child_world_band_rel(t):
    """exp(scaling_child) <=> t with scaling_child = logf(expf(raw) / 1.6f) stored in float32.  expf: 2 U; the divide: U; logf
    returns l within LOGF_REL |l| of ln(d) for the computed d, so |l - ln(exact d)| <= 3 U + 2 U |L|; expf(l) turns that
    absolute error into a relative one and adds its own 2 U.  At the threshold L = ln t: 5 U + 2 U |ln t|, second order added."""
    return 5 * U + LOGF_REL * abs(np.log(float(t))) + 64 * U * U


def thresholds(max_grad, min_opacity, extent, max_screen_size, percent_dense):
    """The host's thresholds: Python doubles, each rounded to float32 once."""
    return {"max_grad": F32(max_grad), "dense_scale": F32(percent_dense * extent), "min_opacity": F32(min_opacity),
            "screen": bool(max_screen_size), "max_screen": F32(max_screen_size if max_screen_size else 0.0),
            "world_scale": F32(0.1 * extent)}


def grads32(accum, denom):
    """:671-672 in float32: one correctly rounded divide, NaN -> 0, inf stays."""
    with np.errstate(invalid="ignore", divide="ignore"):
        g = np.asarray(accum, F32).reshape(-1) / np.asarray(denom, F32).reshape(-1)
    g[np.isnan(g)] = 0
    assert g.dtype == F32
    return g


def decisions(state, thr, densify=True):
    """-> dict of bool [P] masks: clone, split, pruned_self (the row itself and its clone), pruned_child (its children)."""
    scale = np.exp(np.asarray(state["scaling"], np.float64))
    smax = scale.max(axis=1) if scale.shape[0] else np.zeros(0)
    P = scale.shape[0]
    if densify:
        hot = grads32(state["xyz_gradient_accum"], state["denom"]) >= thr["max_grad"]
    else:
        hot = np.zeros(P, bool)
    clone = hot & (smax <= np.float64(thr["dense_scale"]))
    split = hot & (smax > np.float64(thr["dense_scale"]))
    low = sigmoid64(np.asarray(state["opacity"]).reshape(-1)) < np.float64(thr["min_opacity"])
    pruned_self, pruned_child = low.copy(), low.copy()
    if thr["screen"]:
        radii = np.zeros(P, F32) if densify else np.asarray(state["max_radii2D"], F32).reshape(-1)   # the quirk
        pruned_self |= (radii > thr["max_screen"]) | (smax > np.float64(thr["world_scale"]))
        cmax = smax / np.float64(CHILD_SHRINK)
        pruned_child |= (F32(0) > thr["max_screen"]) | (cmax > np.float64(thr["world_scale"]))
    return {"clone": clone, "split": split, "pruned_self": pruned_self, "pruned_child": pruned_child & split}


def in_band(state, thr, densify=True):
    """bool [P]: the row has a decision value inside an ambiguity band of its threshold (every row and every component is
    looked at, whether or not that decision ends up mattering for it)."""
    scale = np.exp(np.asarray(state["scaling"], np.float64))
    bad = np.zeros(scale.shape[0], bool)

    def near(v, t, rel):
        t = np.float64(t)
        return np.abs(v - t) <= rel * abs(t)
    if densify:
        bad |= near(scale, thr["dense_scale"], SCALE_BAND_REL).any(axis=1)
    bad |= near(sigmoid64(np.asarray(state["opacity"]).reshape(-1)), thr["min_opacity"], OPACITY_BAND_REL)
    if thr["screen"]:
        bad |= near(scale, thr["world_scale"], SCALE_BAND_REL).any(axis=1)
        if densify:
            bad |= near(scale / np.float64(CHILD_SHRINK), thr["world_scale"], child_world_band_rel(thr["world_scale"])).any(axis=1)
    return bad


def segments(d):
    """-> (srcA, srcB, srcC): the source index of every row of segments A, B and C (D has C's), in source order."""
    a = np.flatnonzero(~d["split"] & ~d["pruned_self"])
    b = np.flatnonzero(d["clone"] & ~d["pruned_self"])
    c = np.flatnonzero(d["split"] & ~d["pruned_child"])
    return a, b, c


def statistics(d):
    """-> (n_points_cloned, n_points_split, n_points_pruned); the last over the set after clone and split (:690)."""
    pruned = (d["pruned_self"] & ~d["split"]).sum() + (d["clone"] & d["pruned_self"]).sum() \
        + N_CHILDREN * (d["split"] & d["pruned_child"]).sum()
    return int(d["clone"].sum()), int(d["split"].sum()), int(pruned)


# ---- the children's rows ---------------------------------------------------------------------------------------------------

def child_xyz32(raw_q, scale32, noise, xyz):
    """csrc/densify_math.h child_xyz in float32 numpy, operation for operation (numpy's float32 +, *, / are correctly rounded
    and never fused): the norm as param_math.h quat_norm takes it (squares and sums in double, one rounding), q = raw / max(n,
    1e-12), the rows of build_rotation, sample = noise * scale, (R0 s0 + R1 s1) + R2 s2, + xyz.  [n,4],[n,3],[n,3],[n,3] -> [n,3]."""
    rq = np.asarray(raw_q, F32)
    x = rq.astype(np.float64)
    n = np.sqrt(((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2]) + x[:, 3] * x[:, 3]).astype(F32)
    den = np.where(n > F32(1e-12), n, F32(1e-12)).astype(F32)
    q = rq / den[:, None]
    r, qx, qy, qz = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    one, two = F32(1), F32(2)
    R = [[one - two * (qy * qy + qz * qz), two * (qx * qy - r * qz), two * (qx * qz + r * qy)],
         [two * (qx * qy + r * qz), one - two * (qx * qx + qz * qz), two * (qy * qz - r * qx)],
         [two * (qx * qz - r * qy), two * (qy * qz + r * qx), one - two * (qx * qx + qy * qy)]]
    a = np.asarray(noise, F32) * np.asarray(scale32, F32)
    pos = np.asarray(xyz, F32)
    out = np.stack([((R[k][0] * a[:, 0] + R[k][1] * a[:, 1]) + R[k][2] * a[:, 2]) + pos[:, k] for k in range(3)], axis=1)
    assert out.dtype == F32
    return out


def child_xyz64(raw_q, raw_scale, noise, xyz):
    """The same in float64 from the float32 inputs, with the exact exp.  -> (value [n,3], bound [n,3]).
    Bound of the float32 evaluation against it (u = U): q_k carries 2 u (param_math.h); a product of two q's 5 u on a term of
    magnitude <= 1/2, so an off-diagonal entry 2 (ab +- cd) is off by <= 2 (2.5 + 2.5 + 1) u = 12 u and a diagonal one
    1 - 2 (aa + bb) by <= 2 (5 + 1) u + u = 13 u: 16 u absolute with the second order.  sample_j = noise_j * expf(raw_j): 2 u + u.
    R_kj sample_j: (16 + 3 + 1) u |sample_j| with |R_kj| <= 1; the two sums: u each on at most sum_j |sample_j|; the final add:
    u (|xyz_k| + sum_j |sample_j|).  Total <= u (23 sum_j |sample_j| + |xyz_k|); 25 and 2 cover the second order.  A term of
    2^-140 covers roundings that land in the subnormals."""
    x = np.asarray(raw_q, np.float64)
    q = x / np.maximum(np.sqrt((x * x).sum(axis=1)), 1e-12)[:, None]
    r, qx, qy, qz = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.stack([np.stack([1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - r * qz), 2 * (qx * qz + r * qy)], 1),
                  np.stack([2 * (qx * qy + r * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - r * qx)], 1),
                  np.stack([2 * (qx * qz - r * qy), 2 * (qy * qz + r * qx), 1 - 2 * (qx * qx + qy * qy)], 1)], 1)
    a = np.asarray(noise, np.float64) * np.exp(np.asarray(raw_scale, np.float64))
    pos = np.asarray(xyz, np.float64)
    value = np.einsum("nkj,nj->nk", R, a) + pos
    bound = U * (25.0 * np.abs(a).sum(axis=1, keepdims=True) + 2.0 * np.abs(pos)) + 2.0 ** -140
    return value, bound


def child_scaling64(raw_scale):
    """log(exp(raw) / 1.6f) in float64 -> (value, bound).  expf: 2 u relative on the argument of the log = 2 u absolute on its
    value; the divide: u; logf: LOGF_REL of the result.  (3 u + 2 u |L|), second order added."""
    L = np.asarray(raw_scale, np.float64) - np.log(np.float64(CHILD_SHRINK))
    return L, (3 * U + LOGF_REL * np.abs(L)) * (1 + 8 * U)


# ---- the three calls -------------------------------------------------------------------------------------------------------

def _gather(a, src_a, src_new, zero_new):
    a = np.asarray(a)
    new = np.zeros((len(src_new),) + a.shape[1:], a.dtype) if zero_new else a[src_new]
    return np.concatenate([a[src_a], new], axis=0)


def _apply(state, a, b, c, noise, compact):
    """Builds the result from the segments.  state: the six parameters under NAMES, "degrees", "xyz_gradient_accum", "denom",
    "max_radii2D", and optionally "exp_avg" / "exp_avg_sq" / "grad": dicts by name (a missing name: that group has none)."""
    new = np.concatenate([b, c, c])
    nA, nB, nC = len(a), len(b), len(c)
    out = {"src": np.concatenate([a, new]), "nA": nA, "nB": nB, "nC": nC, "P": nA + nB + 2 * nC}
    for name in NAMES:
        out[name] = _gather(state[name], a, new, False)
    out["degrees"] = _gather(state["degrees"], a, new, False)
    for key in ("exp_avg", "exp_avg_sq", "grad"):
        if key in state:
            out[key] = {name: _gather(t, a, new, True) for name, t in state[key].items()}
    if nC:
        child = np.arange(N_CHILDREN).repeat(nC)
        parents = np.concatenate([c, c])
        nz = np.asarray(noise, F32)[child, parents]
        xyz64, xyz_bound = child_xyz64(state["rotation"][parents], state["scaling"][parents], nz, state["xyz"][parents])
        sc64, sc_bound = child_scaling64(state["scaling"][parents])
        out.update(xyz_child64=xyz64, xyz_child_bound=xyz_bound, scaling_child64=sc64, scaling_child_bound=sc_bound)
        # placeholders in the float32 arrays: the children's rows are compared through the float64 values above
        out["xyz"][nA + nB:] = xyz64.astype(F32)
        out["scaling"][nA + nB:] = sc64.astype(F32)
    if compact:
        for key in ("xyz_gradient_accum", "denom", "max_radii2D"):
            out[key] = np.asarray(state[key])[a]
    else:
        out["xyz_gradient_accum"] = np.zeros((out["P"], 1), F32)
        out["density_gradient_accum"] = np.zeros((out["P"], 1), F32)
        out["denom"] = np.zeros((out["P"], 1), F32)
        out["max_radii2D"] = np.zeros(out["P"], F32)
    return out


def densify_and_prune(state, max_grad, min_opacity, extent, max_screen_size, percent_dense, noise):
    """:670-682.  noise: standard normal float32 [2, P, 3], indexed by (child, source Gaussian)."""
    if not max_grad > 0:
        raise ValueError("max_grad must be > 0")
    thr = thresholds(max_grad, min_opacity, extent, max_screen_size, percent_dense)
    d = decisions(state, thr, densify=True)
    out = _apply(state, *segments(d), noise, compact=False)
    out["n_points_cloned"], out["n_points_split"], out["n_points_pruned"] = statistics(d)
    return out


def prune(state, min_opacity, extent, max_screen_size):
    """:684-691 called on its own: the screen-size term sees the real max_radii2D; the accumulators are compacted."""
    thr = thresholds(1.0, min_opacity, extent, max_screen_size, 0.0)
    d = decisions(state, thr, densify=False)
    out = _apply(state, *segments(d), None, compact=True)
    out["n_points_pruned"] = statistics(d)[2]
    return out


def prune_points(state, mask):
    """:553-568."""
    mask = np.asarray(mask, bool)
    none = np.zeros(mask.shape, bool)
    d = {"clone": none, "split": none, "pruned_self": mask, "pruned_child": none}
    return _apply(state, *segments(d), None, compact=True)


def state_bytes(P, M):
    """Bytes of one pass over the state of P Gaussians with M SH coefficients: the six parameters and both moments of each
    (3 x (59 + 3 (M - 1)) floats: 3 x 236 B at M = 16), and _degrees.  The fused call reads and writes it once."""
    return P * (3 * 4 * (3 + 3 + 3 * (M - 1) + 1 + 3 + 4) + 4)


# ---- inputs of the tests ---------------------------------------------------------------------------------------------------
EXTENT, PERCENT_DENSE, MAX_GRAD, MIN_OPACITY = 5.0, 0.01, 0.0002, 0.005   # train.py's defaults on a scene of extent 5


def random_state(P, M, seed, moments=True, grads=False):
    """A model of P Gaussians with M SH coefficients in the reference's shapes, with roughly a quarter of the rows hot, scales
    on both sides of percent_dense * extent and of 0.1 * extent, and opacities on both sides of min_opacity.  A tenth of the
    rows have denom == 0: half of them with a zero accumulator (0/0 -> 0), half with a positive one (inf: selected)."""
    rng = np.random.default_rng(seed)
    s = {"xyz": rng.normal(0, 2, (P, 3)), "f_dc": rng.normal(0, 1, (P, 1, 3)), "f_rest": rng.normal(0, 0.1, (P, M - 1, 3)),
         "opacity": rng.normal(-2, 3, (P, 1)), "scaling": np.log(10.0 ** rng.uniform(-3, 0, (P, 1))) + rng.normal(0, 0.3, (P, 3)),
         "rotation": rng.normal(0, 1, (P, 4)) * 10.0 ** rng.uniform(-1, 1, (P, 1))}
    s = {k: v.astype(F32) for k, v in s.items()}
    s["degrees"] = rng.integers(0, 4, (P, 1)).astype(np.int32)
    denom = rng.integers(1, 90, (P, 1)).astype(F32)
    accum = (denom * 10.0 ** rng.uniform(-5, -3, (P, 1))).astype(F32)
    nothing = rng.random((P, 1)) < 0.1
    denom[nothing] = 0
    accum[nothing & (rng.random((P, 1)) < 0.5)] = 0
    s.update(xyz_gradient_accum=accum, denom=denom, max_radii2D=rng.choice(np.array([0, 3, 17, 40], F32), P).astype(F32))
    for key, on in (("exp_avg", moments), ("exp_avg_sq", moments), ("grad", grads)):
        if on:
            s[key] = {n: (rng.normal(0, 1e-3, s[n].shape) ** (2 if key == "exp_avg_sq" else 1)).astype(F32) for n in NAMES}
    return s


def keep_out_of_bands(state, thr, densify=True):
    """Nudges the rows the generator left inside an ambiguity band out of it (raw scale and raw opacity move by 2^-10, a
    thousand band widths), in place.  The tests assert afterwards that NO row is in a band."""
    for _ in range(8):
        bad = in_band(state, thr, densify)
        if not bad.any():
            break
        state["scaling"][bad] += F32(2.0 ** -10)
        state["opacity"][bad] += F32(2.0 ** -10)
    return state
