#!/usr/bin/env python3
"""Golden vectors of the monotonic alignment search, from the REFERENCE's own compiled ``maximum_path``.

Runs ONLY where a checkout of the reference and Cython exist, once, by hand — never by a test:

    python tests/golden/make_mas_golden.py <path of the reference's Matcha-TTS directory>

``matcha/utils/monotonic_align/core.pyx`` is compiled unmodified into a temporary directory (nothing compiled is kept) and called
through the reference's own wrapper (``monotonic_align/__init__.py``, loaded by file with the compiled ``core`` registered under the
name it imports), on a few small ragged cases: random scores, ``t_x == t_y``, ``t_x == 1``, scores on a coarse grid (many exact
ties), all-equal scores.

Output: tests/golden/mas_vectors.npz — per case ``<name>_value`` (B, Tx, Ty) float32 raw scores, ``<name>_xlen`` / ``<name>_ylen``,
``<name>_path`` int8 and ``<name>_final`` (the DP's value array after the call, float32).
"""
import importlib.util
import os
import subprocess
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True

SETUP = """
from setuptools import setup, Extension
from Cython.Build import cythonize
import numpy
setup(name="mas_core", ext_modules=cythonize([Extension("core", ["core.pyx"], include_dirs=[numpy.get_include()])], language_level=3))
"""


def cases():
    g = torch.Generator().manual_seed(20250311)
    out = {}
    out["random"] = (torch.randn(4, 24, 64, generator=g), [24, 7, 13, 1], [64, 40, 13, 9])
    out["square"] = (torch.randn(3, 17, 17, generator=g) * 3.0, [17, 9, 1], [17, 9, 1])
    out["one_token"] = (torch.randn(2, 1, 37, generator=g), [1, 1], [37, 5])
    out["grid_ties"] = (torch.randint(-2, 3, (4, 12, 40), generator=g).float() * 0.5, [12, 12, 5, 3], [40, 13, 40, 3])
    out["all_equal"] = (torch.full((2, 9, 30), -1.25), [9, 4], [30, 17])
    out["logp_like"] = (-torch.rand(3, 20, 50, generator=g) * 300.0 - 70.0, [20, 11, 2], [50, 49, 50])
    return out


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    pkg = os.path.join(sys.argv[1], "matcha", "utils", "monotonic_align")
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(pkg, "core.pyx"), "rb") as f, open(os.path.join(tmp, "core.pyx"), "wb") as o:
            o.write(f.read())
        with open(os.path.join(tmp, "setup.py"), "w") as o:
            o.write(SETUP)
        subprocess.run([sys.executable, "setup.py", "-q", "build_ext", "--inplace"], cwd=tmp, check=True)
        sys.path.insert(0, tmp)
        core = importlib.import_module("core")
        for name in ("matcha", "matcha.utils", "matcha.utils.monotonic_align"):
            sys.modules.setdefault(name, types.ModuleType(name))
        sys.modules["matcha.utils.monotonic_align.core"] = core
        spec = importlib.util.spec_from_file_location("ref_monotonic_align", os.path.join(pkg, "__init__.py"))
        ma = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(ma)
        out = {}
        for name, (value, xl, yl) in cases().items():
            B, Tx, Ty = value.shape
            xl, yl = torch.tensor(xl), torch.tensor(yl)
            mask = ((torch.arange(Tx)[None, :, None] < xl[:, None, None]) & (torch.arange(Ty)[None, None, :] < yl[:, None, None])).float()
            path = ma.maximum_path(value, mask)                                  # the reference's wrapper, its own masking and lengths
            final = (value * mask).numpy().astype(np.float32)                    # ... and the value array its loop leaves behind
            core.maximum_path_c(np.zeros(final.shape, np.int32), final, xl.numpy().astype(np.int32), yl.numpy().astype(np.int32))
            assert path.dtype == torch.float32 and tuple(path.shape) == (B, Tx, Ty)
            out[f"{name}_value"] = value.numpy().astype(np.float32)
            out[f"{name}_xlen"], out[f"{name}_ylen"] = xl.numpy().astype(np.int32), yl.numpy().astype(np.int32)
            out[f"{name}_path"] = path.numpy().astype(np.int8)
            out[f"{name}_final"] = final
            print(f"{name}: {tuple(value.shape)} lengths {xl.tolist()} / {yl.tolist()}  frames on the path {int(path.sum())}")
    dst = os.path.join(HERE, "mas_vectors.npz")
    np.savez_compressed(dst, **out)
    print(f"wrote {dst} ({os.path.getsize(dst) / 1024:.0f} KB)")


if __name__ == "__main__":
    main()
