"""r3dgs_quantised -- the quantised model, resident on the device as it is stored in the file.

The reference's `save_ply(quantised=True)` (scene/gaussian_model.py:239-311) writes one byte per attribute -- an index into
one of twenty 256-entry codebooks -- plus the position as float or half, grouped by SH degree; its `load_ply` inflates all of
it to dense fp32 again (236 B per Gaussian, every SH row padded to degree 3) before anything is rendered.  A `QuantisedModel`
keeps the ids, the positions and the codebooks as they are (at most 62 B per Gaussian) and the rasterizer reads them in
place (`diff_gaussian_rasterization._C.rasterize_gaussians_quantised`, include/r3dgs_quantised.h):

    from r3dgs_quantised import QuantisedModel
    from r3dgs_render import render
    qm = QuantisedModel.from_ply("point_cloud_quantised_half.ply", half_float=True)
    image = render(view, qm, pipe, background)["render"]

Fine-tuning in codebook space: the ids stay fixed, the 20 x 256 centres and the positions are the parameters.

    qm.requires_grad_(codebooks=True, xyz=True)      # qm.codebooks becomes a leaf; qm.xyz_master [P,3] float32 is created
    opt = r3dgs_optim.Adam(qm.parameters(), lr=1e-3)  # (or torch.optim.Adam)
    out = render(view, qm, pipe, background)          # differentiable in qm.codebooks and qm.xyz_master
    loss(out["render"], target).backward(); opt.step()
    qm.commit(); qm.to_ply("point_cloud_quantised_half.ply")

With grad enabled, render() of a trainable model decodes the ids into dense tensors that live for that step
(`_C.quantised_decode`), runs the raw-parameter training route of r3dgs_render on them, and its backward sums the decoded
tensors' gradients into the centres (`_C.quantised_codebook_grad`: double accumulation in a fixed order, no atomics -- the
same inputs give the same bits) and hands the position gradient through.  The resident model stays as small as it was.
A model nobody asked gradients of, or any model under no_grad, renders through the in-place inference route as before.
The SH-sparsity term (lambda_sh_sparsity) is not available for a quantised model.
"""
import os
from collections import OrderedDict

import numpy as np
import torch

from diff_gaussian_rasterization import _C

BOOK_NAMES = (["features_dc"] + [f"features_rest_{i}" for i in range(15)] +
              ["opacity", "scaling", "rotation_re", "rotation_im"])   # the rows of `codebooks`, the file's order
GEOM_COLUMNS = ["opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"]   # the columns of `geom_ids`
DECODED = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation", "_degrees")


class QuantisedModel:
    """xyz float16 / float32 [P,3] -- geom_ids uint8 [P,8] (GEOM_COLUMNS) -- sh_ids uint8, ragged: Gaussian i of degree d
    owns 3 (d+1)^2 bytes, [coefficient][channel] -- codebooks float32 [20,256] (BOOK_NAMES) -- band tables int32 [4].
    Gaussians are sorted by degree.  No array is padded."""

    def __init__(self, xyz, geom_ids, sh_ids, codebooks, per_band_count, max_sh_degree=3):
        if max_sh_degree != 3 or len(per_band_count) != 4:
            raise ValueError("a quantised model has 4 bands (SH degrees 0..3)")
        if tuple(codebooks.shape) != (20, 256):
            raise ValueError(f"a quantised model has 20 codebooks of 256 centres, got {tuple(codebooks.shape)}")
        self.per_band_count = [int(c) for c in per_band_count]
        P = sum(self.per_band_count)
        want = sum(3 * (d + 1) ** 2 * c for d, c in enumerate(self.per_band_count))
        if tuple(xyz.shape) != (P, 3) or tuple(geom_ids.shape) != (P, 8) or tuple(sh_ids.shape) != (want,):
            raise ValueError("quantised model: array shapes do not match the per-degree counts")
        dev = xyz.device
        self.xyz, self.geom_ids, self.sh_ids = xyz.contiguous(), geom_ids.contiguous(), sh_ids.contiguous()
        self.codebooks = codebooks.to(device=dev, dtype=torch.float32).contiguous()
        i32 = dict(dtype=torch.int32, device=dev)
        self.per_band = torch.tensor(self.per_band_count, **i32)
        self.cumsum = torch.cumsum(self.per_band, dim=0).to(torch.int32)
        self.coeffs = torch.tensor([1, 4, 9, 16], **i32)
        self.max_sh_degree = self.active_sh_degree = 3
        self.xyz_master = None   # float32 [P,3] leaf while the positions are trained (requires_grad_)

    # ---- construction ------------------------------------------------------------------------------------------------
    @classmethod
    def from_ply(cls, path, half_float, max_sh_degree=3, device="cuda"):
        """Reads the reference's quantised file straight into the arrays above (no dense tensor is built).  `half_float`
        as given to save_ply: positions and centres are half bit patterns stored as int16."""
        from plyfile import PlyData
        ply = PlyData.read(path)
        names = [e.name for e in ply.elements]
        if "codebook_centers" not in names:
            raise ValueError(f"{path}: no codebook_centers element -- not a quantised file (save_ply(quantised=True))")
        if max_sh_degree != 3 or names != [f"vertex_{d}" for d in range(4)] + ["codebook_centers"]:
            raise ValueError(f"{path}: expected vertex_0..vertex_3 (4 bands) and codebook_centers, found {names}")
        centres = ply.elements[-1]
        if centres.count != 256:
            raise ValueError(f"{path}: {centres.count} centres per codebook; only 256 are supported")
        ftype = np.int16 if half_float else np.float32

        def floats(a):   # file column -> float16 (bit-cast) or float32 array
            a = np.ascontiguousarray(np.asarray(a, dtype=ftype))
            return a.view(np.float16) if half_float else a
        books = np.stack([floats(centres[n]).astype(np.float32) for n in BOOK_NAMES])   # half centres widened once, exactly
        xyz, geom, sh, counts = [], [], [], []
        for d in range(4):
            g, cn = ply.elements[d], (d + 1) ** 2 - 1
            n = g.count
            counts.append(n)
            xyz.append(np.stack([floats(g[k]) for k in "xyz"], axis=1).reshape(n, 3))
            geom.append(np.stack([np.asarray(g[k], dtype=np.uint8) for k in GEOM_COLUMNS], axis=1).reshape(n, 8))
            dc = np.stack([np.asarray(g[f"f_dc_{c}"], dtype=np.uint8) for c in range(3)], axis=1).reshape(n, 1, 3)
            if cn:   # the file holds rrr.. ggg.. bbb..: [channel][coefficient] -> [coefficient][channel]
                rest = np.stack([np.asarray(g[f"f_rest_{j}"], dtype=np.uint8) for j in range(3 * cn)], axis=1)
                dc = np.concatenate([dc, rest.reshape(n, 3, cn).transpose(0, 2, 1)], axis=1)
            sh.append(dc.reshape(-1))
        dev = torch.device(device)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
        return cls(t(np.concatenate(xyz)), t(np.concatenate(geom)), t(np.concatenate(sh)), t(books), counts)

    @classmethod
    def from_gaussian_model(cls, pc, half_float=True):
        """From a clustered model of the reference (pc._codebook_dict of produce_clusters, pc._degrees, pc._xyz), sorted by
        degree exactly as save_ply writes it; `half_float` rounds positions and centres to half as save_ply does."""
        cb = pc._codebook_dict
        if cb is None or list(cb.keys()) != BOOK_NAMES:
            raise ValueError("the model has no codebooks (produce_clusters) or not the reference's twenty")
        for n in BOOK_NAMES:
            if cb[n].centers.numel() != 256:
                raise ValueError(f"codebook {n}: {cb[n].centers.numel()} centres; only 256 are supported")
        deg = pc._degrees.reshape(-1)
        order = torch.cat([torch.nonzero(deg == d).reshape(-1) for d in range(4)])
        counts = [int((deg == d).sum()) for d in range(4)]
        ids = lambda n: cb[n].ids.reshape(deg.numel(), -1).to(torch.uint8)[order]   # noqa: E731
        geom = torch.cat([ids("opacity"), ids("scaling"), ids("rotation_re"), ids("rotation_im")], dim=1)
        full = torch.stack([ids("features_dc")] + [ids(f"features_rest_{i}") for i in range(15)], dim=1)   # [P,16,3]
        sh, first = [], 0
        for d, c in enumerate(counts):
            sh.append(full[first:first + c, :(d + 1) ** 2].reshape(-1))
            first += c
        books = torch.stack([cb[n].centers.detach().reshape(256).float() for n in BOOK_NAMES])
        xyz = pc._xyz.detach()[order]
        if half_float:
            xyz, books = xyz.half(), books.half().float()
        else:
            xyz = xyz.float()
        return cls(xyz, geom, torch.cat(sh), books, counts)

    # ---- what it is ----------------------------------------------------------------------------------------------------
    @property
    def P(self):
        return int(self.xyz.shape[0])

    @property
    def xyz_is_half(self):
        return self.xyz.dtype == torch.float16

    @property
    def device(self):
        return self.xyz.device

    @property
    def nbytes(self):
        """Resident bytes: P (8 + 6 or 12) + sum_d 3 (d+1)^2 P_d + 20 * 256 * 4 + 48 (band tables); nothing is padded."""
        return _C.quantised_bytes(self.P, self.per_band_count, self.xyz_is_half)

    def arrays(self):
        """(xyz, geom_ids, sh_ids, codebooks, per_band, cumsum, coeffs): the positional model arguments of
        _C.rasterize_gaussians_quantised / _C.quantised_decode, in the order the latter takes them."""
        return self.xyz, self.geom_ids, self.sh_ids, self.codebooks, self.per_band, self.cumsum, self.coeffs

    def decode(self):
        """The dense tensors the reference's load_ply returns for this model (bands above a Gaussian's degree decode to
        centre 0 of their codebook, as there), decoded on the device: {_xyz, _features_dc, _features_rest, _opacity,
        _scaling, _rotation, _degrees}."""
        if self.device.type != "cuda":
            raise RuntimeError("QuantisedModel.decode: the model is on the host; the decoder runs on the device (no CPU path)")
        return OrderedDict(zip(DECODED, _C.quantised_decode(*self.arrays())))

    # ---- fine-tuning: the centres and the positions as parameters, the ids fixed -----------------------------------------
    @property
    def trainable(self):
        return bool(self.codebooks.requires_grad) or self.xyz_master is not None

    def requires_grad_(self, codebooks=True, xyz=True):
        """Asks for gradients of the centres and / or the positions.  `codebooks` (float32 [20,256]) becomes a leaf.  For the
        positions a float32 leaf `xyz_master` [P,3] is created from the exact widening of `xyz`; the stored `xyz` is not
        touched while training (a half array trained in place would round every step away) -- commit() rounds it back."""
        self.codebooks = self.codebooks.detach().requires_grad_(bool(codebooks))
        if xyz:
            if self.xyz_master is None:
                self.xyz_master = self.xyz.detach().to(torch.float32).clone().requires_grad_(True)
        else:
            self.xyz_master = None
        return self

    def parameters(self):
        """The optimizer's parameter groups (r3dgs_optim.Adam, torch.optim.Adam): only what requires_grad_ asked for."""
        groups = []
        if self.codebooks.requires_grad:
            groups.append({"params": [self.codebooks], "name": "codebooks"})
        if self.xyz_master is not None:
            groups.append({"params": [self.xyz_master], "name": "xyz"})
        return groups

    def decode_for_training(self):
        """(xyz, features_dc, features_rest, opacity, scaling, rotation, degrees) for one training step: decode()'s tensors,
        differentiable in `codebooks`; xyz is `xyz_master` itself when the positions are trained (they are then not decoded)."""
        if self.device.type != "cuda":
            raise RuntimeError("QuantisedModel: the model is on the host; the decoder runs on the device (no CPU path)")
        out = _DecodeQuantised.apply(self.codebooks, self, self.xyz_master is None)
        xyz = self.xyz_master if self.xyz_master is not None else out[6]
        return (xyz,) + tuple(out[:6])

    def commit(self, half_float=None):
        """Ends a fine-tune: rounds xyz_master into xyz's dtype (as .half() does), rounds the centres to half-representable
        floats when `half_float` (default: when the positions are half, as in a half_float file), and drops the leaves.
        Afterwards the inference forward renders exactly the committed values."""
        half = self.xyz_is_half if half_float is None else bool(half_float)
        with torch.no_grad():
            if self.xyz_master is not None:
                self.xyz = self.xyz_master.detach().to(self.xyz.dtype).contiguous()
            books = self.codebooks.detach()
            self.codebooks = (books.half().float() if half else books.clone()).contiguous()
        self.xyz_master = None
        return self

    def to_ply(self, path, half_float=None):
        """Writes the reference's quantised file (the layout of its save_ply(quantised=True), read back by from_ply):
        vertex_0..vertex_3 with x y z, the id bytes f_dc_*, f_rest_* (rrr.. ggg.. bbb..), opacity, scale_*, rot_*, then
        codebook_centers.  half_float (default: whether the positions are half): positions and centres as half bit patterns
        in int16 columns.  With the model's own format, from_ply gives every array back bit for bit."""
        from plyfile import PlyData, PlyElement
        if self.trainable:
            raise RuntimeError("QuantisedModel.to_ply: the model is being trained; commit() first")
        half = self.xyz_is_half if half_float is None else bool(half_float)
        ftype = "i2" if half else "f4"

        def floats(t):   # float tensor -> the file's column: half bit patterns as int16, or float32
            t = t.detach().cpu()
            return t.half().view(torch.int16).numpy() if half else t.float().numpy()
        xyz, geom, sh = floats(self.xyz), self.geom_ids.cpu().numpy(), self.sh_ids.cpu().numpy()
        elements, first, byte = [], 0, 0
        for d, n in enumerate(self.per_band_count):
            K = (d + 1) ** 2
            ids = sh[byte:byte + 3 * K * n].reshape(n, K, 3)
            rest = ids[:, 1:, :].transpose(0, 2, 1).reshape(n, 3 * (K - 1))   # [coefficient][channel] -> [channel][coefficient]
            columns = ([(k, ftype, xyz[first:first + n, j]) for j, k in enumerate("xyz")] +
                       [(f"f_dc_{c}", "u1", ids[:, 0, c]) for c in range(3)] +
                       [(f"f_rest_{j}", "u1", rest[:, j]) for j in range(3 * (K - 1))] +
                       [(k, "u1", geom[first:first + n, j]) for j, k in enumerate(GEOM_COLUMNS)])
            el = np.empty(n, dtype=[(k, t) for k, t, _ in columns])
            for k, _, col in columns:
                el[k] = col
            elements.append(PlyElement.describe(el, f"vertex_{d}"))
            first, byte = first + n, byte + 3 * K * n
        books = floats(self.codebooks)
        centres = np.empty(256, dtype=[(n, ftype) for n in BOOK_NAMES])
        for k, n in enumerate(BOOK_NAMES):
            centres[n] = books[k]
        elements.append(PlyElement.describe(centres, "codebook_centers"))
        if os.path.dirname(path):
            os.makedirs(os.path.dirname(path), exist_ok=True)
        PlyData(elements).write(path)


class _DecodeQuantised(torch.autograd.Function):
    """codebooks -> (features_dc, features_rest, opacity, scaling, rotation, degrees[, xyz]) of a QuantisedModel by
    _C.quantised_decode; the backward is its adjoint, _C.quantised_codebook_grad."""

    @staticmethod
    def forward(ctx, codebooks, qm, want_xyz):
        xyz, dc, rest, opacity, scaling, rotation, degrees = _C.quantised_decode(
            qm.xyz, qm.geom_ids, qm.sh_ids, codebooks, qm.per_band, qm.cumsum, qm.coeffs, want_xyz=want_xyz)
        ctx.ids = (qm.geom_ids, qm.sh_ids, qm.per_band, qm.cumsum, qm.coeffs)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(degrees)
        if not want_xyz:
            return dc, rest, opacity, scaling, rotation, degrees
        ctx.mark_non_differentiable(xyz)
        return dc, rest, opacity, scaling, rotation, degrees, xyz

    @staticmethod
    def backward(ctx, g_dc, g_rest, g_opacity, g_scaling, g_rotation, *_):
        grads = [None if g is None else g.contiguous() for g in (g_dc, g_rest, g_opacity, g_scaling, g_rotation)]
        return _C.quantised_codebook_grad(*ctx.ids, *grads), None, None
