"""Time CommitmentKey.setup on the device: wall time and the library's own split (mira_set_timing) into the host's SHAKE256
squeeze, the hash kernel and the map kernel, per curve and key size.

    python tools/setup_timing.py [--k 20 24] [--repeat 2] [--chunk POINTS]

One JSON line per run.  setup_squeeze_host is host time; setup_hash and setup_map are device intervals summed over the chunks
(a chunk's hash interval includes its wait for the squeeze and upload of its stream bytes).  hash_kernel_ms and map_kernel_ms
are the two kernels alone, over 2^k messages already in device memory (mira_hash_to_field_device, mira_map_to_curve_device)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def kernels_alone(lib, curve, k):
    import ctypes

    import numpy as np
    n = 1 << k
    d_m, d_u = lib.alloc(n * 32), lib.alloc(n * 64)
    try:
        lib.upload(d_m, np.random.default_rng(k).integers(0, 256, n * 32, dtype=np.uint8))
        lib.check(lib.c.mira_set_timing(1))
        lib.check(lib.c.mira_hash_to_field_device(curve, ctypes.c_void_p(d_m), n, ctypes.c_void_p(d_u)))
        out = {"hash_kernel_ms": dict(lib.timings())["setup_hash"]}
        lib.check(lib.c.mira_map_to_curve_device(curve, ctypes.c_void_p(d_u), n, ctypes.c_void_p(d_u)))
        out["map_kernel_ms"] = dict(lib.timings())["setup_map"]
        lib.check(lib.c.mira_set_timing(0))
        return out
    finally:
        lib.free(d_m)
        lib.free(d_u)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, nargs="+", default=[20, 24])
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--chunk", type=int, default=-1)
    args = ap.parse_args()
    from mira_amd import _lib
    from mira_amd import commitment as cm
    lib = _lib.load()
    lib.tune(_lib.TUNE_SETUP_CHUNK, args.chunk)
    for curve in (cm.CURVE_BN256, cm.CURVE_GRUMPKIN):
        cm.CommitmentKey.setup(curve, 12, b"warm-up").close()              # code objects loaded, pinned buffers seen once
        for k in args.k:
            for rep in range(args.repeat):
                lib.check(lib.c.mira_set_timing(1))
                t0 = time.perf_counter()
                key = cm.CommitmentKey.setup(curve, k, b"timing")          # returns after the streams have drained
                wall = time.perf_counter() - t0
                stages = dict(lib.timings())
                lib.check(lib.c.mira_set_timing(0))
                key.close()
                if rep == 0:
                    stages.update(kernels_alone(lib, curve, k))
                print(json.dumps(dict(curve=curve, k=k, rep=rep, chunk=args.chunk, wall_ms=round(wall * 1e3, 2),
                                      **{name: round(ms, 2) for name, ms in stages.items()})), flush=True)


if __name__ == "__main__":
    main()
