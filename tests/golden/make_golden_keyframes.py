#!/usr/bin/env python
"""Regenerates tests/golden/keyframe_nearest.npz.  BUILD container only (needs /root/reference):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_keyframes.py

Inputs and results of the reference's own torch_consecutive_nearest1d (nr3d_lib/utils.py:675-699; pure torch, on the CPU) for the
cases of tests/dynamic_march_ref.py::golden_cases: per case `<name>.keys`, `<name>.t`, and the three returned tensors
`<name>.inds` (int64), `<name>.mask` (bool), `<name>.dis` (float32).  Data only."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True

import numpy as np
import torch

from make_golden import import_reference   # noqa: E402
import dynamic_march_ref as ref   # noqa: E402


def main():
    utils = import_reference("nr3d_lib.utils")
    out = {}
    for name, keys, t in ref.golden_cases():
        inds, mask, dis = utils.torch_consecutive_nearest1d(torch.from_numpy(keys.copy()), torch.from_numpy(t.copy()))
        out.update({f"{name}.keys": keys, f"{name}.t": t, f"{name}.inds": inds.numpy().astype(np.int64),
                    f"{name}.mask": mask.numpy(), f"{name}.dis": dis.numpy().astype(np.float32)})
    path = os.path.join(HERE, "keyframe_nearest.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out) // 5} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
