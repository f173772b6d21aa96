"""Counting experiment (R3DG_EXP_COUNT build): one M1 step, then the device counters.
R3DG_LIB_DIR=exp/COUNT/lib python tools/exp_count.py"""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import relightable3dgaussian_amd as r3  # noqa: E402

sys.argv = ["bench.py", "--steps", "1", "--warmup", "0", "--full", "--no-cpu-baseline"]
bench.main()
lib = ctypes.CDLL(os.path.join(r3.LIB_DIR, "libr3dg_hip.so"))
buf, fb = (ctypes.c_ulonglong * 4)(), (ctypes.c_ulonglong * 4)()
lib.r3dg_exp_counters_bwd(buf)
lib.r3dg_exp_counters_fwd(fb)
print(f"bwd live pairs: {buf[0]}\nbwd mfma groups: {buf[1]}")
# bench.main runs the warm-up steps, the timed steps and as many profiled steps: 2 at --steps 1
print("m1 steps run: 2")
print(f"fwd steps done: {fb[2]}\nfwd live pairs (pre-exit): {fb[3]}")
# walk iterations (a pair or an odd count's one-visit tail each): 2 x iterations - steps = the tails, which
# were predicated-off second steps ("phantoms") before the tail had a body of its own
print(f"bwd walk iterations: {buf[2]}\nbwd one-visit tails: {2 * buf[2] - buf[0]}")
print(f"fwd walk iterations: {fb[0]}\nfwd one-visit tails: {2 * fb[0] - fb[2]}")
