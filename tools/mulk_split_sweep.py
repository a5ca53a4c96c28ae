#!/usr/bin/env python3
"""A/B sweep behind the launch-shape switch of poly_mul_ntt_k
and, with --kl, of poly_mul_ntt_kl at l = 2.

Takes two builds of the library, one that never spreads the rows over
gridDim.y and one that always does:

    make HIPFLAGS='-O3 -std=c++17 --offload-arch=gfx950 -fPIC -DMULK_SPLIT_FORCE=0' LIB=lib/split0.so lib/split0.so
    make HIPFLAGS='-O3 -std=c++17 --offload-arch=gfx950 -fPIC -DMULK_SPLIT_FORCE=1' LIB=lib/split1.so lib/split1.so
    python tools/mulk_split_sweep.py lib/split0.so lib/split1.so [out.json]

(--kl: -DMULKL_SPLIT_FORCE=0 / 1 builds) and times both in one process,
alternating, over half-octave batches 1 .. 16384 (7 x 200 launches per point,
HIP events, outputs compared).  The switch (mulk_split_max, csrc/ntt_mulk.hpp;
mulkl_split_max, csrc/ntt_mulkl.hpp) is the largest batch at which the split
shape is the faster one.
"""
import ctypes
import json
import sys

import numpy as np
import torch

vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int


def load(path):
    L = ctypes.CDLL(path)
    L.poly_mul_ntt_k.argtypes = [vp, vp, vp, vp, sz, ci, ci, vp]
    L.poly_mul_ntt_kl.argtypes = [vp, ctypes.POINTER(vp), vp, vp, sz, ci, ci, ci, vp]
    L.ntt_fill_uniform.argtypes = [vp, sz, ci, ctypes.c_uint64, ctypes.c_uint64, vp]
    return L


def main():
    argv = [a for a in sys.argv[1:] if a != "--kl"]
    l = 2 if "--kl" in sys.argv[1:] else 1
    libs = {0: load(argv[0]), 1: load(argv[1])}
    dev = torch.device("cuda:0")
    n_of = {0: 1024, 1: 1024, 2: 2048}
    res = []
    batches = sorted({int(round(2 ** (e / 2))) for e in range(0, 29)})
    for ps, k in ((1, 4), (2, 5), (0, 4), (2, 2), (1, 8)):
        n = n_of[ps]
        for batch in batches:
            ys = [torch.empty(batch * n, dtype=torch.int32, device=dev) for _ in range(l)]
            a = torch.empty(k * l * n, dtype=torch.int32, device=dev)
            out = [torch.empty(batch * k * n, dtype=torch.int32, device=dev) for _ in (0, 1)]
            for j, y in enumerate(ys):
                libs[0].ntt_fill_uniform(y.data_ptr(), batch, ps, 1 + 16 * j, 0, None)
            libs[0].ntt_fill_uniform(a.data_ptr(), k * l, ps, 2, 0, None)
            s = torch.cuda.current_stream().cuda_stream
            inner = 200 if batch <= 2048 else 50
            py = (vp * l)(*[y.data_ptr() for y in ys])

            def run(v, cnt):
                for _ in range(cnt):
                    if l == 1:
                        rc = libs[v].poly_mul_ntt_k(out[v].data_ptr(), ys[0].data_ptr(), a.data_ptr(), None, batch, k, ps, s)
                    else:
                        rc = libs[v].poly_mul_ntt_kl(out[v].data_ptr(), py, a.data_ptr(), None, batch, k, l, ps, s)
                    assert rc == 0, rc

            for v in (0, 1):
                run(v, 20)
            torch.cuda.synchronize()
            assert torch.equal(out[0], out[1])
            t = {0: [], 1: []}
            for _ in range(7):
                for v in (0, 1):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    run(v, inner)
                    e1.record()
                    e1.synchronize()
                    t[v].append(e0.elapsed_time(e1) * 1e3 / inner)
            m = {v: float(np.median(t[v])) for v in t}
            row = dict(ps=ps, k=k, l=l, batch=batch, us_nosplit=round(m[0], 3), us_split=round(m[1], 3),
                       spread_nosplit=round(max(t[0]) - min(t[0]), 3), spread_split=round(max(t[1]) - min(t[1]), 3),
                       ratio=round(m[0] / m[1], 3))
            res.append(row)
            print(json.dumps(row), flush=True)
    if len(argv) > 2:
        json.dump(res, open(argv[2], "w"), indent=0)


if __name__ == "__main__":
    main()
