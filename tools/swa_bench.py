"""Times mmr_swin_window_attention at the Swin-T stage 2-4 geometries (B = 256, as in the cfg2
step) with whichever libmmr MMR_LIBMMR selects; HIP events, random operands.  Diagnostic only.
SWA_PINS=0,1 alternates the routes (mmr_pin_variant MMR_PIN_SWA: 0 gather kernel, 1 streaming kernel)
over SWA_ROUNDS rounds in one process and prints, per geometry and route, the median
and the spread of the rounds, GB/s of bytes in + out, and whether the output bits equal route 0's.
usage: [MMR_LIBMMR=...] [SWA_B=256] [SWA_PINS=0,1] python tools/swa_bench.py [tag]"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import mmr_amd  # noqa: E402,F401
from mmr_amd import ops  # noqa: E402

B = int(os.environ.get("SWA_B", "256"))
PINS = [int(p) for p in os.environ["SWA_PINS"].split(",")] if os.environ.get("SWA_PINS") else [None]
ROUNDS = int(os.environ.get("SWA_ROUNDS", "5" if PINS != [None] else "1"))
tag = sys.argv[1] if len(sys.argv) > 1 else ""


def timed(f):
    f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 20 * 1e3


row = []
for H, heads, shift in [(28, 6, 0), (28, 6, 3), (14, 12, 0), (14, 12, 3), (7, 24, 0)]:
    C = heads * 32
    qkv = torch.randn(B, H, H, 3 * C, device="cuda").to(torch.bfloat16)
    bias = ops.swin_attn_bias(torch.randn(169, heads, device="cuda"), heads, 7, H, shift)
    if os.environ.get("SWA_Q8") == "1":  # the MX-fp8-emitting form (fp8 stages)
        f = lambda: ops.swin_window_attention_q8(qkv, bias, H, heads, 7, shift)  # noqa: E731
    else:
        f = lambda: ops.swin_window_attention(qkv, bias, H, heads, 7, shift)  # noqa: E731
    nbytes = B * H * H * 4 * C * 2
    if PINS == [None]:
        us = timed(f)
        row.append(f"H{H}s{shift} {us:6.1f}us {nbytes / us / 1e3:5.0f}GB/s")
        continue
    us = {p: [] for p in PINS}
    same = {}
    for rd in range(ROUNDS):
        for p in PINS:
            with ops.pinned(ops.PIN_SWA, p):
                us[p].append(timed(f))
                if rd == 0 and os.environ.get("SWA_Q8") != "1":
                    y = f()
                    if p == PINS[0]:
                        y0 = y
                    same[p] = bool(torch.equal(y.view(torch.int16), y0.view(torch.int16)))
    for p in PINS:
        med = statistics.median(us[p])
        print(f"{tag} B{B} H{H} heads{heads} shift{shift} pin{p}: median {med:6.1f} us  min {min(us[p]):6.1f} max "
              f"{max(us[p]):6.1f}  {nbytes / med / 1e3:5.0f} GB/s  bits==pin{PINS[0]}: {same.get(p)}", flush=True)
if row:
    print(tag, " | ".join(row), flush=True)
