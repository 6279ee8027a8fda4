"""The colour role of the quantised forward (csrc/preprocess.hip color_role_quant) through every kernel instance that
carries it, with workgroups that do more than one round, and over models whose arrays sit only at the alignment
validate_forward demands.  tests/test_quantised_gpu.py renders models of at most two 256-Gaussian chunks, all of which the
default plan hands to the third carrier; here every model has five chunks.

Two references.  Bit for bit: the fp32 ragged inference forward of decode() (test_quantised_gpu's ragged_inputs /
ragged_forward / assert_same_pass).  Independent: the CPU oracle over the model decoded in numpy (tests/quant_ref.py
np_decode), at test_gpu_parity.check_forward's existing bars -- the ragged and the quantised colour roles share their
walk over the chunks, so a mistake there is one they could share.  A colour chunk nobody evaluates keeps the r = g = b = 0
the geometry kernel wrote, so every visible Gaussian of a skipped chunk changes the image.

What reaches what (chunks of 256 Gaussians; default split 25 / 45 / 30 % -> carrier_chunks):

  test_models_put_visible_gaussians_where_the_paths_need_them (CPU)
      the condition the GPU tests stand on, from the oracle alone: every 64-row wave of every model shows a Gaussian, the
      first and the last row (the one-row tail waves among them) do, every degree shows in the carrier it falls in, some
      Gaussians are culled
  test_every_carrier_against_both_references[model]
      depth_sort_color_quant_kernel<0> (chunk 0), <1> (chunks 1-2), <2> (chunks 3-4), each workgroup one round, on the
      exact path and on the reserved path (capture, then graph replay).  mixed: degree changes inside waves of carriers 1
      and 2 whose spans start off a 16-byte boundary (head != 0), a last wave of one row that ends at the array's last byte
      (byte-wise tail chunk).  all3: the longest spans (3072 B, 192 chunks: three loads in every lane), head == 0 and no
      byte-wise chunk.  all0: 192-byte spans (12 chunks, lanes 12..63 load nothing), the byte-wise tail.  front3: every
      degree inside wave 0 of carrier 0, every later span off a 16-byte boundary.  float_xyz: quant_xyz's fp32 loads
  test_counter_mode_through_every_carrier
      the same launches in counter mode (the geometry kernel's counters beside the colour role)
  test_model_at_its_required_alignment_only[model]
      sh_ids 1, 7 and 15 bytes off a 16-byte boundary: wave 0 has head != 0 and its first chunk reaches in front of the
      array's first byte (byte-wise head chunk), the tail chunk reaches behind its last; geom_ids at 8, codebooks at 16,
      xyz at one element: the uint2 load of preprocess_geom_kernel<5>, the float4 copy of the books into LDS, quant_xyz.
      Guard bytes around every array, rewritten between runs, show that no byte outside an array reaches a result
  test_refused_alignments
      validate_forward's refusal of what is below that alignment, on both paths
  test_forced_plans_equal_the_default_plan (child processes: the knobs are read once per process)
      R3DGS_DEPTH_SORT=generic R3DGS_COLOR_GRID=2   preprocess_color_quant_kernel, two workgroups of three and two rounds
      R3DGS_COLOR_GRID=1 R3DGS_COLOR_SPLIT0=100      <0> carries all five chunks in one workgroup: five rounds, the id
                                                    window reused behind the trailing barrier, one copy of the books
      R3DGS_COLOR_GRID=1 R3DGS_COLOR_SPLIT0=0 R3DGS_COLOR_SPLIT1=100   the same in <1>
      R3DGS_COLOR_GRID=1                             default split, <1> and <2> two rounds each, `first + wg < last`
                                                    with a single workgroup

The models are qr.make_model's with half positions and half centres, but for two centres of each SH codebook: the largest
finite halves (+-65504), which make_model plants among its special halves, are replaced by +-1.5.  check_forward's colour
bar is absolute (1e-5, made for colours of order one); with those centres the oracle's own image of `mixed` reaches 4.4e4,
where fp32 values lie 4e-3 apart, so no fp32 blend could be held to that bar whatever it computes.  The zeros, subnormals,
the smallest normal and one stay."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import synth_scene as ss
from tests import quant_ref as qr
from tests import test_gpu_parity as gp
from tests import test_quantised_gpu as tq

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMAGE = "131x77"   # partial tiles
BG = np.array([0.1, 0.2, 0.3], np.float32)   # tq.camera's background
SCALES = (1.0, 0.5)
CHUNK = 256        # csrc/common.h kPreBlock
# per-degree counts, the seed of qr.make_model (fixed by the CPU test below, never on the card)
MODELS = {
    "mixed": dict(counts=(300, 290, 280, 283), seed=1),      # 4 * 256 + 129 = 18 * 64 + 1
    "all3": dict(counts=(0, 0, 0, 1100), seed=2),
    "all0": dict(counts=(1100, 0, 0, 0), seed=5),            # (seed 3 culls row 0)
    "front3": dict(counts=(1, 1, 1, 1150), seed=4),
    "float_xyz": dict(counts=(300, 290, 280, 283), seed=1, half_xyz=False),   # mixed with fp32 positions
}
CHILD_MODELS = ("mixed", "all3")
ENVIRONMENTS = (
    dict(R3DGS_DEPTH_SORT="generic", R3DGS_COLOR_GRID="2"),
    dict(R3DGS_COLOR_GRID="1", R3DGS_COLOR_SPLIT0="100"),
    dict(R3DGS_COLOR_GRID="1", R3DGS_COLOR_SPLIT0="0", R3DGS_COLOR_SPLIT1="100"),
    dict(R3DGS_COLOR_GRID="1"),
)
KNOBS = ("R3DGS_DEPTH_SORT", "R3DGS_COLOR_GRID", "R3DGS_COLOR_SPLIT0", "R3DGS_COLOR_SPLIT1")


def carrier_chunks(P, split0=25, split1=45):
    """[(first, last)) colour chunks of the histogram, scatter and bucket-sort launches: what issue_depth_sort_and_color
    (csrc/preprocess.hip) computes from the split that make_fwd_plan (csrc/pass_driver.hip) sets -- 25 / 45 / 30 % up to
    2^20 Gaussians unless R3DGS_COLOR_SPLIT0 / 1 say otherwise, the second share cut where the two exceed 100."""
    chunks = (P + CHUNK - 1) // CHUNK
    if split0 + split1 > 100:
        split1 = 100 - split0
    c1 = chunks * split0 // 100
    c2 = c1 + chunks * split1 // 100
    return [(0, c1), (c1, c2), (c2, chunks)]


_host = {}


def host_model(name, tame=True):
    """The model's numpy arrays; the cloud sits 4 units in front of the camera, as test_quantised_gpu places it."""
    if (name, tame) not in _host:
        kw = MODELS[name]
        m = qr.make_model(kw["counts"], seed=kw["seed"], half_xyz=kw.get("half_xyz", True), half_centres=True,
                          centre=(0.0, 0.0, 4.0), spread=0.8)
        if tame:   # (module docstring) the two largest finite halves among the SH centres
            big = np.abs(m["codebooks"][:16]) == 65504.0
            assert big.sum() == 32
            m["codebooks"][:16][big] = np.sign(m["codebooks"][:16][big]) * 1.5
        _host[(name, tame)] = m
    return _host[(name, tame)]


def host_camera():
    W, H, f, seed = tq.IMAGES[IMAGE]
    return ss.make_camera(W, H, f, seed), W, H


def host_activations(d):
    """csrc/param_math.h scale_act and quat_act in numpy, for the test that has no device: exp, and q / max(|q|, eps) with
    the norm taken in double.  (The GPU tests hand the oracle _C.activate_params's values instead.)"""
    raw = d["_rotation"].astype(np.float64)
    n = np.sqrt((raw * raw).sum(axis=1, keepdims=True)).astype(np.float32)
    return np.exp(d["_scaling"]).astype(np.float32), (d["_rotation"] / np.maximum(n, np.float32(1e-12))).astype(np.float32)


def oracle_of(m, scale, activations):
    """The CPU oracle's forward of the model decoded in numpy."""
    d = qr.np_decode(m)
    scales, rotations = activations(d)
    g = dict(means3D=d["_xyz"], opacity=d["_opacity"], scales=scales, rotations=rotations, degrees=d["_degrees"],
             sh=np.ascontiguousarray(np.concatenate((d["_features_dc"], d["_features_rest"]), axis=1)))
    cam, W, H = host_camera()
    return gp.oracle_forward(BG, g, cam, H, W, mod=scale)


def assert_model_conditions(name, m, ref):
    """What makes a render of the model a test of every wave of every carrier."""
    vis = ref["radii"] > 0
    P = sum(m["counts"])
    assert vis.shape == (P,) and (~vis).any(), "some Gaussians must be culled"
    for w0 in range(0, P, 64):   # only a tail wave shorter than 8 rows is exempt
        assert P - w0 < 8 or vis[w0:w0 + 64].any(), f"{name}: no visible Gaussian in the wave at {w0}"
    # the chunks at the two ends of sh_ids, put together byte by byte where they reach past the array, belong to these rows
    assert vis[0] and vis[P - 1], f"{name}: the first and the last row must show"
    if name in ("mixed", "front3", "float_xyz"):
        assert P % 64 == 1, "the tail wave holds a single row"
    if name == "front3":
        assert vis[:3].all(), "the three low-degree rows in front of wave 0"
    deg = np.repeat(np.arange(4), m["counts"])
    shares = carrier_chunks(P)
    assert [hi - lo for lo, hi in shares] == [1, 2, 2], shares   # five chunks; every carrier has a share
    for k, (lo, hi) in enumerate(shares):
        rows = slice(lo * CHUNK, min(hi * CHUNK, P))
        for d in np.unique(deg[rows]):
            assert (vis[rows] & (deg[rows] == d)).any(), f"{name}: degree {d} does not show in carrier {k}"


def test_models_put_visible_gaussians_where_the_paths_need_them():
    assert carrier_chunks(5 * CHUNK, 100, 45) == [(0, 5), (5, 5), (5, 5)] and carrier_chunks(1153, 0, 100) == [(0, 0), (0, 5), (5, 5)]
    for name in MODELS:
        m = host_model(name)
        sh_bytes = sum(3 * (d + 1) ** 2 * c for d, c in enumerate(m["counts"]))
        assert m["sh_ids"].size == sh_bytes and m["xyz"].dtype == (np.float32 if name == "float_xyz" else np.float16)
        for scale in SCALES:
            assert_model_conditions(name, m, oracle_of(m, scale, host_activations))
    a, b = host_model("mixed"), host_model("float_xyz")
    assert all(np.array_equal(a[k], b[k]) for k in ("geom_ids", "sh_ids", "codebooks"))
    assert np.array_equal(a["xyz"], b["xyz"].astype(np.float16)) and not np.array_equal(a["xyz"].astype(np.float32), b["xyz"])


# ---- on the device ---------------------------------------------------------------------------------------------------
_device, _refs = {}, {}


def device_model(name):
    """(QuantisedModel in arrays of its own, its numpy arrays); built once and left unchanged."""
    if name not in _device:
        _device[name] = (tq.device_model(host_model(name)), host_model(name))
    return _device[name]


def oracle_ref(_C, name, scale):
    """The oracle's forward with the DEVICE's activations (tests/test_sh_rows_gpu.py case), once per (model, scale)."""
    if (name, scale) not in _refs:
        def activations(d):
            act = _C.activate_params(tq._dev(d["_scaling"]), tq._dev(d["_rotation"]))
            return act[0].cpu().numpy(), act[1].cpu().numpy()
        m = host_model(name)
        _refs[(name, scale)] = oracle_of(m, scale, activations)
        assert_model_conditions(name, m, _refs[(name, scale)])
    return _refs[(name, scale)]


def reservation(out):
    return int(out[0].pairs * 1.25) + 4096


def reserved_twice(_C, qm, c, scale, reserve):
    """The reserved path twice (the second call replays the graph the first captured); neither may be redone."""
    before = _C.pass_stats()
    outs = [tq.quantised_forward(_C, qm, c, scale, exact=False, reserve=reserve) for _ in range(2)]
    after = _C.pass_stats()
    assert after["reserved_passes"] == before["reserved_passes"] + 2 and after["redone_passes"] == before["redone_passes"]
    assert all(o[0].ticket > 0 for o in outs), "the reserved path was not taken"
    return outs


@gpu
@pytest.mark.parametrize("name", list(MODELS))
def test_every_carrier_against_both_references(name):
    from diff_gaussian_rasterization import _C
    qm, _ = device_model(name)
    c = tq.camera(IMAGE)
    inputs = tq.ragged_inputs(_C, qm)
    for scale in SCALES:
        ref = oracle_ref(_C, name, scale)
        want = tq.ragged_forward(_C, qm, inputs, c, scale)
        got = tq.quantised_forward(_C, qm, c, scale)
        tq.assert_same_pass(_C, qm.P, c, got, want, (name, scale, "exact"))
        gp.check_forward(_C, got, ref, c.H, c.W, qm.P)
        reserve = reservation(want)
        want_r = tq.ragged_forward(_C, qm, inputs, c, scale, exact=False, reserve=reserve)
        for n, got_r in enumerate(reserved_twice(_C, qm, c, scale, reserve)):
            tq.assert_same_pass(_C, qm.P, c, got_r, want_r, (name, scale, "reserved", n))
            gp.check_forward(_C, got_r, ref, c.H, c.W, qm.P)


@gpu
def test_counter_mode_through_every_carrier():
    from diff_gaussian_rasterization import _C
    qm, _ = device_model("mixed")
    c = tq.camera(IMAGE)
    (want, t_w, m_w), (got, t_g, m_g) = tq.counter_passes(_C, qm, c)
    tq.assert_same_pass(_C, qm.P, c, got, want, "counter mode")
    assert t_w.sum() > 0 and torch.equal(t_g, t_w), "out_touched_pixels"
    assert (m_w > 0).any() and torch.equal(m_g > 0, m_w > 0)
    for lo, hi in carrier_chunks(qm.P):
        assert (t_w[lo * CHUNK:hi * CHUNK] > 0).any(), "every carrier's Gaussians must be counted"
    assert ((m_g - m_w).abs() <= tq.transmittance_rounding(c, m_w)).all(), "out_transmittance"


GUARD = 64


class Embedded:
    """An array as a view into a larger device buffer: [GUARD + lead bytes][the array][GUARD bytes], one allocation."""

    def __init__(self, a, lead):
        a = np.ascontiguousarray(a)
        self.first, self.last = GUARD + lead, GUARD + lead + a.nbytes
        self.buf = torch.full((self.last + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 256 == 0, "the offsets below are counted from an aligned allocation"
        self.buf[self.first:self.last] = torch.from_numpy(a.view(np.uint8).reshape(-1)).cuda()
        dtype = getattr(torch, a.dtype.name)
        self.view = self.buf[self.first:self.last].view(dtype).view(a.shape)   # (torch refuses a view off its element size)

    def fill_guards(self, value, as_float=False):
        for part in (self.buf[:self.first], self.buf[self.last:]):
            (part.view(torch.float32) if as_float else part).fill_(value)

    def holds(self, t):
        return t.data_ptr() == self.buf.data_ptr() + self.first


def embedded_model(m, sh_lead, geom_lead=8, books_lead=16, xyz_lead=None):
    from r3dgs_quantised import QuantisedModel
    parts = dict(xyz=Embedded(m["xyz"], m["xyz"].itemsize if xyz_lead is None else xyz_lead), geom_ids=Embedded(m["geom_ids"], geom_lead),
                 sh_ids=Embedded(m["sh_ids"], sh_lead), codebooks=Embedded(m["codebooks"], books_lead))
    qm = QuantisedModel(parts["xyz"].view, parts["geom_ids"].view, parts["sh_ids"].view, parts["codebooks"].view, m["counts"])
    return qm, parts


def both_paths(_C, qm, c, reserve):
    return [tq.quantised_forward(_C, qm, c)] + reserved_twice(_C, qm, c, 1.0, reserve)


@gpu
@pytest.mark.parametrize("name", ["mixed", "all0", "float_xyz"])
def test_model_at_its_required_alignment_only(name):
    from diff_gaussian_rasterization import _C
    own, m = device_model(name)
    c = tq.camera(IMAGE)
    want = tq.quantised_forward(_C, own, c)
    reserve = reservation(want)
    decoded = qr.np_decode(m)
    for sh_lead in (1, 7, 15):
        qm, parts = embedded_model(m, sh_lead)
        # QuantisedModel kept the views (.contiguous() of a contiguous slice is the slice): the offsets survived
        for k, t in (("xyz", qm.xyz), ("geom_ids", qm.geom_ids), ("sh_ids", qm.sh_ids), ("codebooks", qm.codebooks)):
            assert parts[k].holds(t), k
        assert qm.sh_ids.data_ptr() % 16 == sh_lead and qm.geom_ids.data_ptr() % 16 == 8 and qm.codebooks.data_ptr() % 32 == 16
        assert qm.xyz.data_ptr() % (2 * m["xyz"].itemsize) == m["xyz"].itemsize
        # guards as built (0xA5), then 0x00, then 0xFF -- around the codebooks a huge float
        for fill in (None, 0x00, 0xFF):
            for k, e in parts.items():
                if fill == 0xFF and k == "codebooks":
                    e.fill_guards(3.0e38, as_float=True)
                elif fill is not None:
                    e.fill_guards(fill)
            for n, got in enumerate(both_paths(_C, qm, c, reserve)):
                tq.assert_same_pass(_C, qm.P, c, got, want, (name, sh_lead, fill, n))
            d = qm.decode()
            for k in qr.KEYS:
                g = d[k].cpu().numpy()
                assert g.shape == decoded[k].shape and g.dtype == decoded[k].dtype, k
                assert np.array_equal(qr.bits(g), qr.bits(decoded[k])), (name, sh_lead, fill, k)


@gpu
def test_refused_alignments():
    """Below the alignment validate_forward demands (geom_ids 8 bytes: one uint2 load; codebooks 16: float4 loads; xyz its
    element) the call is refused before anything is launched, on the exact and on the reserved path."""
    from diff_gaussian_rasterization import _C
    _, m = device_model("mixed")
    c = tq.camera(IMAGE)
    cases = [dict(geom_lead=4), dict(books_lead=4)]
    try:   # a half view at an odd byte: torch does not build one (storage offsets count in elements), so nothing can pass it on
        Embedded(m["xyz"], 1)
    except RuntimeError:
        pass
    else:
        cases.append(dict(xyz_lead=1))
    for kw in cases:
        qm, _ = embedded_model(m, 0, **kw)
        for exact in (True, False):
            with pytest.raises(RuntimeError, match="geom_ids must be 8-byte aligned, codebooks 16-byte, xyz to its element"):
                tq.quantised_forward(_C, qm, c, exact=exact, reserve=None if exact else 100000)
    tq.quantised_forward(_C, embedded_model(m, 0)[0], c)   # the same construction at the required alignment passes


# ---- the forced plans: one fresh process per environment ---------------------------------------------------------------
def pass_arrays(_C, P, c, out):
    """Everything compared between two passes, as numpy arrays."""
    a = dict(image=out[1].cpu().numpy(), radii=out[2].cpu().numpy(), counts=np.array([int(out[0]), out[0].pairs], np.int64))
    assert not out[0].truncated and out[0].pairs > 0
    for k, v in _C.export_binning(P, out[0], c.H, c.W, out[3], out[4], out[5]).items():
        a[k] = v.cpu().numpy()
    return a


def child_check(npz):
    """Run in a child process under one of ENVIRONMENTS: the quantised entry on the exact and on the reserved path equals
    the default plan's recorded pass bit for bit, and is held to the oracle by check_forward."""
    from diff_gaussian_rasterization import _C
    recorded = np.load(npz)
    c = tq.camera(IMAGE)
    for name in CHILD_MODELS:
        qm, _ = device_model(name)
        for scale in SCALES:
            ref = oracle_ref(_C, name, scale)
            exact = tq.quantised_forward(_C, qm, c, scale)
            for n, out in enumerate([exact] + reserved_twice(_C, qm, c, scale, reservation(exact))):
                got = pass_arrays(_C, qm.P, c, out)
                for k, v in got.items():
                    w = recorded[f"{name}/{scale}/{k}"]
                    assert v.shape == w.shape and v.dtype == w.dtype and np.array_equal(qr.bits(v), qr.bits(w)), (name, scale, n, k)
                gp.check_forward(_C, out, ref, c.H, c.W, qm.P)


@gpu
def test_forced_plans_equal_the_default_plan(tmp_path):
    from diff_gaussian_rasterization import _C
    assert not any(k in os.environ for k in KNOBS), "this process must be on the default plan"
    c = tq.camera(IMAGE)
    recorded = {}
    for name in CHILD_MODELS:
        qm, _ = device_model(name)
        for scale in SCALES:
            out = tq.quantised_forward(_C, qm, c, scale)
            gp.check_forward(_C, out, oracle_ref(_C, name, scale), c.H, c.W, qm.P)
            for k, v in pass_arrays(_C, qm.P, c, out).items():
                recorded[f"{name}/{scale}/{k}"] = v
    npz = str(tmp_path / "default_plan.npz")
    np.savez(npz, **recorded)
    code = ("import sys\n"
            "sys.path[:0] = [%r, %r]\n"
            "from tests import test_quantised_paths_gpu as t\n"
            "t.child_check(%r)\n"
            "print('quantised-paths-ok')\n") % (ROOT, os.path.join(ROOT, "reduced-3dgs_amd"), npz)
    for extra in ENVIRONMENTS:   # one at a time; the first child that fails ends the test, no further one is started
        try:
            out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **extra), capture_output=True, text=True,
                                 cwd=ROOT, timeout=180)
        except subprocess.TimeoutExpired as e:
            pytest.fail(f"{extra}: timed out\n{str(e.stdout)[-2000:]}\n{str(e.stderr)[-2000:]}")
        assert out.returncode == 0 and "quantised-paths-ok" in out.stdout, \
            f"{extra}: exit {out.returncode}\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}"
