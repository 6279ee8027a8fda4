"""Writes the quantised-model fixtures of tests/test_quantised_cpu.py / test_quantised_gpu.py:

    quantised_half_P200.ply, quantised_P200.ply   the reference's own save_ply(quantised=True, half_float=True / False)
    quantised_P200_loaded.npz                     what the reference's load_ply returns for each of them

    python tests/golden/make_quantised_golden.py /path/to/reference

Run once, in the authoring container: the reference's scene/gaussian_model.py runs unmodified on this repository's
plyfile / simple_knn / diff_gaussian_rasterization, on the CPU (`torch.Tensor.cuda` is made a no-op because that code
hard-codes `.cuda()`), the way tests/test_plyfile_shim.py runs it.  Everything written is data of the reference's programs."""
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
COUNTS = (37, 13, 80, 70)   # Gaussians of degree 0..3 (shuffled in the model: save_ply sorts them)


def main(ref):
    sys.path[:0] = [ref, os.path.join(ROOT, "reduced-3dgs_amd"), ROOT]
    torch.Tensor.cuda = lambda self, *a, **k: self
    if not hasattr(np, "cast"):   # np.cast[np.float16](..) (gaussian_model.py:269) left NumPy in 2.0
        class _Cast:
            def __getitem__(self, dtype):
                return lambda a: np.asarray(a, dtype=dtype)
        np.cast = _Cast()
    import scene.gaussian_model as gm
    g = torch.Generator().manual_seed(11)
    P = sum(COUNTS)
    deg = torch.cat([torch.full((c,), d, dtype=torch.int32) for d, c in enumerate(COUNTS)])
    deg = deg[torch.randperm(P, generator=g)].reshape(P, 1)
    m = gm.GaussianModel(3)
    m._degrees = deg
    # a cloud in front of the golden cameras (tests/golden_cases.py): the GPU tests render it
    m._xyz = torch.randn(P, 3, generator=g) * 0.6

    def book(cols, centres):
        return gm.Codebook(torch.randint(0, 256, (P, cols), generator=g, dtype=torch.uint8), centres.reshape(256, 1))
    cb = OrderedDict()
    cb["features_dc"] = book(3, torch.randn(256, generator=g))
    for i in range(15):
        cb[f"features_rest_{i}"] = book(3, torch.randn(256, generator=g) * 0.3)
    cb["opacity"] = book(1, torch.randn(256, generator=g) * 2.0)
    cb["scaling"] = book(3, torch.randn(256, generator=g) * 0.5 - 2.5)
    cb["rotation_re"] = book(1, torch.randn(256, generator=g))
    cb["rotation_im"] = book(3, torch.randn(256, generator=g))
    m._codebook_dict = cb
    loaded = {}
    for half, name in ((True, "quantised_half_P200"), (False, "quantised_P200")):
        path = os.path.join(HERE, name + ".ply")
        m.save_ply(path, quantised=True, half_float=half)
        back = gm.GaussianModel(3)
        back.load_ply(path, half_float=half, quantised=True)
        for k in ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation", "_degrees"):
            loaded[("half" if half else "float") + k] = getattr(back, k).detach().numpy()
        print(path, os.path.getsize(path), "bytes")
    out = os.path.join(HERE, "quantised_P200_loaded.npz")
    np.savez_compressed(out, **loaded)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
