#!/usr/bin/env python3
"""Time per call of sv_farthest_point_sampling (fixed layout, 24 scenes, one workgroup per scene) at one size per tier of k_fps_reg and for
k_fps_stream: the instantiations the bucket and several-workgroup kernels otherwise keep out of tools/fps_micro.py.  SEEVCN_LIB selects the library."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from seevcn_amd import _lib
lib = _lib.load()
dev = torch.device("cuda:0")
rng = np.random.default_rng(0)
for n, m, tier in ((2048, 1024, "reg<4>"), (4096, 1024, "reg<8>"), (8192, 1024, "reg<16>"), (16384, 1024, "reg<32>"), (20480, 1024, "reg<40>"), (24576, 1024, "reg<48>"), (30000, 256, "stream")):
    b = 24
    x = torch.from_numpy((rng.normal(size=(b, n, 3)) * 20).astype(np.float32)).to(dev)
    temp = torch.empty((b, n), dtype=torch.float32, device=dev)
    idx = torch.empty((b, m), dtype=torch.int32, device=dev)
    call = lambda: _lib.check(lib.sv_farthest_point_sampling(_lib.ptr(x), b, n, m, _lib.ptr(temp), _lib.ptr(idx), _lib.stream()), "fps")
    call(); call(); torch.cuda.synchronize()
    ms = []
    for _ in range(5):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(3):
            call()
        e.record(); e.synchronize()
        ms.append(s.elapsed_time(e) / 3)
    ms.sort()
    print(f"tier k_fps_{tier:8s} {b} x {n} -> {m}: median {ms[2]:8.3f} ms  min {ms[0]:8.3f}  max {ms[-1]:8.3f}  ({ms[2] / m * 1e3:.2f} us/round)  checksum {int(idx.long().sum())}", flush=True)
