#!/usr/bin/env python
"""Write tests/golden/lepe_long.json by running the REAL reference at the long stripe windows (225 .. 512 tokens):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_lepe_long.py --ref <checkout of the reference>

For every LePEAttention window of tests/lepe_long_cases.py, its two CSWinBlocks and the 384 px CSWinTransformer the reference module is
built under the case's seed protocol, converted to fp64 and run on the CPU (eval, no_grad); the fixture keeps fp64 checksums (sum,
sum |.|), the shapes and the 257 strided samples of cases.sample_index -- no full tensors.  tests/test_lepe_long_cpu.py holds the
oracle (oracle/cswin.py, fp64) against it.  Runs only where a checkout of the reference exists, like make_golden.py.
"""
import argparse
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests"), HERE):
    sys.path.insert(0, p)

from cases import sample_index  # noqa: E402
import lepe_long_cases as LC  # noqa: E402


def record(x, y):
    yf = y.double().reshape(-1)
    return {"x_shape": list(x.shape), "x_sum": float(x.double().sum()), "y_shape": list(y.shape), "sum": float(yf.sum()),
            "abs_sum": float(yf.abs().sum()), "samples": [float(v) for v in yf[sample_index(yf.numel())]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference (the directory that holds vision_transformers/)")
    args = ap.parse_args()
    sys.dont_write_bytecode = True
    sys.path.insert(0, args.ref)
    from vision_transformers.cswin import CSWinBlock, CSWinTransformer, LePEAttention
    out = {"torch": torch.__version__, "protocol": "tests/lepe_long_cases.py builders on the reference classes, eval, fp64 CPU", "cases": {}}

    def run(cid, m, x):
        with torch.no_grad():
            y = m.double()(x.double())
        out["cases"][cid] = record(x, y)
        print(f"{cid:28s} sum={out['cases'][cid]['sum']:.9f} abs={out['cases'][cid]['abs_sum']:.6f}")

    for case in LC.WINDOWS:
        run("lepe_" + LC.wid(case), *LC.lepe_inputs(LePEAttention, case))
    for row in LC.BLOCKS:
        run("block_" + row[0], *LC.block_inputs(CSWinBlock, row))
    run("model_384", *LC.model_inputs(CSWinTransformer))
    with open(os.path.join(HERE, "lepe_long.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
