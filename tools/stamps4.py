#!/usr/bin/env python3
"""Diagnostic (GPU box, library built with EEM_EXTRA_FLAGS=-DEEM_STAMPS=<C>, C = 16 / 32 / 64): where a wave of wino4_kernel
(conv_wino4.hip) spends its cycles - the stamps of the last launch with that channel count (median over blocks).
    tools/stamps4.py [frames]      frames per launch (default 1; 10 is the timed configuration's launch)
A k-step in five parts: wait + barrier | DMA issue | patch reads + column pass | row passes + MFMAs | (per tile) epilogue.  With
EEM_W4_VSHARE on, the third part is empty for the MFMA waves and the duty pass (patch reads, both passes, V writes) is its own column."""
import ctypes, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eemflow_amd import _lib
from eemflow_amd.weights import seeded_state_dict, synthetic_voxel_pair
B = int(sys.argv[1]) if len(sys.argv) > 1 else 1
L = _lib.lib()
dev = torch.device("cuda", 0)
flat = torch.cat([torch.from_numpy(v).reshape(-1) for v in seeded_state_dict(0).values()]).contiguous()
c = ctypes.c_void_p(); _lib.check(L.eemflow_create(0, ctypes.byref(c)))
_lib.check(L.eemflow_load_weights(c, flat.data_ptr(), flat.numel(), 5, 5))
H, W = 720, 1280
_lib.check(L.eemflow_set_image_size(c, H, W, None)); _lib.check(L.eemflow_use_graph(c, 0))
e1, e2 = (torch.from_numpy(a).to(dev) for a in synthetic_voxel_pair(1, B, H, W))
out = torch.empty(B, 2, H, W, device=dev)
for _ in range(3):
    _lib.check(L.eemflow_forward(c, e1.data_ptr(), e2.data_ptr(), B, H, W, out.data_ptr(), H, W, None))
torch.cuda.synchronize()
NS = 128
n = 1024 * 8 * NS
buf = (ctypes.c_ulonglong * n)()
L.eemflow_debug_read_stamps4.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
assert L.eemflow_debug_read_stamps4(buf, n) == 0
s = np.frombuffer(buf, dtype=np.uint64).reshape(1024, 8, NS).astype(np.int64)       # the LAST wino4 launch wrote these: pconv3_3
nb = int((s[:, 0, 0] > 0).sum())
s = s[:nb]
ks = int(((s[0, 0, 2:60] > 0).sum()) // 2)
vshare = bool((s[:, :, 65] > s[:, :, 3]).all())                                     # the duty pass comes after the MFMAs, the column pass before
print("frames per launch", B, " shared V:", vshare)
print('tiles per block (by k-steps): ', sorted(set(((s[:, 0, 2:60] > 0).sum(axis=1) // 2).tolist())))
print("blocks", nb, "k-steps stamped", ks)
med = lambda v: int(np.median(v))
for w in (0, 7):
    a = s[:, w]
    t0 = a[:, 0]
    print(f"wave {w}: prologue {med(a[:, 1] - t0)}")
    prev = a[:, 1]
    tot = np.zeros(5)
    for l in range(min(ks, 16)):
        b, d, cp, e = a[:, 2 + 2 * l], a[:, 64 + 2 * l], a[:, 65 + 2 * l], a[:, 3 + 2 * l]
        if vshare:      # barrier | DMA | MFMAs | duty pass
            parts = (med(b - prev), med(d - b), 0, med(e - d), med(cp - e))
            end = cp
        else:
            parts = (med(b - prev), med(d - b), med(cp - d), med(e - cp), 0)
            end = e
        tot += parts
        print(f"   k-step {l:2d}: wait+barrier {parts[0]:6d}  DMA issue {parts[1]:5d}  patch+columns {parts[2]:5d}  rows+MFMAs {parts[3]:6d}  duty pass {parts[4]:5d}")
        prev = end
    if ks >= 16:
        epi = med(a[:, 62] - prev)
        allc = tot.sum() + epi
        print(f"   tile 0: wait+barrier {tot[0]:.0f} ({100 * tot[0] / allc:.1f} %)  DMA issue {tot[1]:.0f} ({100 * tot[1] / allc:.1f} %)  patch+columns {tot[2]:.0f} ({100 * tot[2] / allc:.1f} %)"
              f"  rows+MFMAs {tot[3]:.0f} ({100 * tot[3] / allc:.1f} %)  duty pass {tot[4]:.0f} ({100 * tot[4] / allc:.1f} %)  epilogue {epi} ({100 * epi / allc:.1f} %)  sum {allc:.0f}")
    print(f"   total {med(a[:, 60] - t0)} cycles, {med(a[:, 61])} ticks of 10 ns -> {np.median((a[:, 60] - t0) / np.maximum(a[:, 61], 1)) / 10:.2f} GHz")
ran = (s[:, :, 0] > 0) & (s[:, :, 60] > 0)                                          # (a block without a tile returns before its first stamp)
t_start, t_end = s[:, :, 0][ran], s[:, :, 60][ran]
print("first start -> last end", int(t_end.max() - t_start.min()), "cycles; start spread", int(t_start.max() - t_start.min()))
