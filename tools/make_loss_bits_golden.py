#!/usr/bin/env python
"""Writes tests/golden/loss_bits/loss_bits_small.npz: what the loss entry points of csrc/loss.hip write, bit for bit, on the inputs of
tests/loss_bits_cases.py -- recorded from a build of the commit whose bits are the contract, so that a later change of the kernel
file can be held to them (tests/test_loss_bits_gpu.py).  Needs the GPU.  One precision per process (vl-bert_amd/_lib.py), so the tool
runs itself once per build and merges:

    python tools/make_loss_bits_golden.py [--lib-dir DIR]      # DIR: where libvlbert_hip.so / libvlbert_hip_f16.so of that commit lie

The file holds only arrays the library wrote (and the list of their names).  Equal arrays are stored once: `keys[i]` names an output,
`blob_of[i]` the `blob_<n>` that holds it -- the DS / ACC / logits_copy forms of one entry point write the same gradient.
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "loss_bits", "loss_bits_small.npz")


def record(path):
    from tests import loss_bits_cases as LB
    got = {}
    for name in LB.CASES:
        for k, v in LB.run(name).items():
            got[LB.precision() + "/" + k] = v
    np.savez(path, **got)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib-dir", default=os.path.join(ROOT, "vl-bert_amd"))
    ap.add_argument("--record", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.record:
        return record(args.record)
    merged = {}
    with tempfile.TemporaryDirectory() as tmp:
        for prec, lib in (("bf16", "libvlbert_hip.so"), ("f16", "libvlbert_hip_f16.so")):
            part = os.path.join(tmp, prec + ".npz")
            env = dict(os.environ, VLB_PRECISION=prec, VLB_LIB_PATH=os.path.join(os.path.abspath(args.lib_dir), lib))
            subprocess.run([sys.executable, os.path.abspath(__file__), "--record", part], env=env, cwd=ROOT, check=True, timeout=300)
            with np.load(part) as z:
                merged.update({k: z[k] for k in z.files})
    keys, blobs, blob_of, seen = sorted(merged), [], [], {}
    for k in keys:
        v = merged[k]
        ident = (v.dtype.str, v.shape, v.tobytes())
        if ident not in seen:
            seen[ident] = len(blobs)
            blobs.append(v)
        blob_of.append(seen[ident])
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, keys=np.array(keys), blob_of=np.array(blob_of, dtype=np.int32), **{"blob_%d" % i: b for i, b in enumerate(blobs)})
    print("%s: %d outputs in %d arrays, %d bytes" % (os.path.relpath(OUT, ROOT), len(keys), len(blobs), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
