"""Records tests/golden/tail_slots_parent.npz: what pn2x_add_layernorm_perm of the LOADED library returns for the exact-integer
inputs of tests/test_gpu_tail_slots.py (B = 1, j = 21, re = 5, c = 384 -- the network's shape -- ldz = re * c + 4), with and
without bias and the second LayerNorm.  Run once on an MI355X with the library of the commit before the slot count became a
compile-time value (ca6fb1e); the test holds every later kernel to these bits.
usage: python tests/golden/make_golden_tail_slots.py <out.npz>   (from the repository root; needs a GPU)"""
import ctypes
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
spec = importlib.util.spec_from_file_location("tail_slots_cases", os.path.join(os.path.dirname(HERE), "test_gpu_tail_slots.py"))
cases = importlib.util.module_from_spec(spec)
spec.loader.exec_module(cases)

from hotrack_amd import ext  # noqa: E402  (the library under record: the working directory's package)

B, j, re, c, pad = 1, 21, 5, 384, 4
z, bias, aff = cases.exact_inputs(B, j, re, c, pad)
perm = cases.table(j, re)
dz, dbias, daff = z.cuda(), bias.cuda(), [a.cuda() for a in aff]
rec = {"B": B, "j": j, "re": re, "c": c, "pad": pad}
p = cases._p
for use_ln2 in (False, True):
    for use_bias in (False, True):
        out = torch.full((B * j, c), cases.SENTINEL, device="cuda")
        rc = ext._lib.pn2x_add_layernorm_perm(B, j, re, c, p(dz), dz.stride(0), p(perm), p(dbias if use_bias else None), p(daff[0]),
                                              p(daff[1]), cases.EPS1, p(daff[2] if use_ln2 else None),
                                              p(daff[3] if use_ln2 else None), cases.EPS2 if use_ln2 else 0.0, p(out), None)
        assert rc == 0
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.isfinite(got).all()
        rec[f"out_ln2{int(use_ln2)}_bias{int(use_bias)}"] = got
np.savez_compressed(sys.argv[1], **rec)
print("wrote", sys.argv[1], {k: getattr(v, "shape", v) for k, v in rec.items()})
