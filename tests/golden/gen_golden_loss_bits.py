#!/usr/bin/env python
"""Records tests/golden/g16_loss_bits.npz: the output bits of every csrc/loss.hip kernel on the
cases of tests/loss_bits_cases.py (inputs from an integer formula, outputs only in the file).

Run ONCE on the MI355X against a build of the commit BEFORE a change that must keep the bits (the
fixture in the tree was taken from the parent of the commit that added it), loaded the way
tools/ab_libs.sh loads a baseline:

    LD_LIBRARY_PATH=abtest/parent DSTAGNN_EXT=$PWD/abtest/parent/_C.so \
        python tests/golden/gen_golden_loss_bits.py [--out FILE]

A bit that differs afterwards is a reordered add or a changed contraction in the new code: the
fixture is not re-recorded for it.
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))          # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))  # the repository

import loss_bits_cases as cases  # noqa: E402
from dstagnn_drought_amd import _lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "g16_loss_bits.npz"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gen_golden_loss_bits.py records on the GPU only: no HIP device")
    ops, dev = _lib.load(), torch.device("cuda:0")
    out = {}
    for group, fn in cases.GROUPS.items():
        got = fn(ops, dev)
        assert got and all(k.startswith(cases.PREFIX[group]) for k in got), group
        assert not set(got) & set(out)
        again = fn(ops, dev)  # the premise: the same bits on every launch
        for k, v in got.items():
            v = v.detach().cpu().contiguous()
            assert torch.equal(v.view(torch.int32), again[k].cpu().contiguous().view(torch.int32)), k
            out[k] = v.numpy()
    stat = torch.from_numpy(out["cap/mae/stat"])
    dy, want = cases.grid_cap_dy(ops, dev, stat)
    assert torch.equal(dy.view(torch.int32), want.view(torch.int32)), "mae dy is not sign(y - t) * scale"
    np.savez_compressed(a.out, **out)
    size = os.path.getsize(a.out)
    print(f"{a.out}: {len(out)} arrays, {size} bytes")
    assert size < 200 * 1024, "the fixture must stay under 200 KB"


if __name__ == "__main__":
    main()
