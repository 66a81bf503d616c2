"""How much of a bench frame the elevated-only compaction kernel does not have to load (csrc/ground.hip: it skips an aligned group of 8 input points — a
128-byte line of the cloud — that holds no point which can be elevated, and a whole 64-point wave item with a scalar branch): the share of elevated-free
8-groups and 64-tiles on the GPU's OWN frames, from the masks mot_get_ground returns, and the share the kernel's conservative test (the group's max z against
every lane's threshold) reaches, recomputed from what it is handed: the group words (mot_debug_copy 16), the cells (17) and the thresholds (10).
    python tools/skip_share.py [streams] [--scene street|plaza] [--point-order beam|firing|random]
profiles/ground_skip.md sets the figures beside the 63 % / 52 % of the CPU renderer's frames."""
import argparse, ctypes as C, importlib.util, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path, submodule_search_locations=[os.path.dirname(path)])
    m = importlib.util.module_from_spec(spec); sys.modules[name] = m; spec.loader.exec_module(m); return m
ap = argparse.ArgumentParser()
ap.add_argument("streams", type=int, nargs="?", default=16)
ap.add_argument("--scene", choices=("street", "plaza"), default="street")
ap.add_argument("--point-order", choices=("beam", "firing", "random"), default="beam")
a = ap.parse_args()
import torch
torch.cuda.init()
PKG = os.path.join(ROOT, "3d-lidar-multi-object-tracking_amd")
mot = _load("mot_amd", os.path.join(PKG, "__init__.py")); sdev = _load("mot_amd.synth_dev", os.path.join(ROOT, "tools", "synth", "synth_dev.py"))
B, N, F = a.streams, 120000, 4
stride = ((N + 2047) // 2048) * 2048
v, yaw = sdev.load_ego(F)
seq, n_seq, _, _ = sdev.SequenceRenderer("cuda").render(list(range(B)), F, N, stride, v, yaw, scene=a.scene, order=a.point_order)
ELEV, DROPPED = 2, 0
tot = {8: [0, 0], 64: [0, 0]}; cons = {8: [0, 0], 64: [0, 0]}; pts = [0, 0]
MARGIN = float(mot.params(0).ground_margin)
with mot.Context(max_points=stride, max_batch=B) as c:
    for f in (0, F - 1):
        c.frames_dev(seq[f].data_ptr(), stride * 4, n_seq[f]); c.synchronize()
        for b in range(B):
            n = int(n_seq[f][b]); m = c.get_ground(b, n_hint=n)["mask"]
            pts[0] += int((m == ELEV).sum()); pts[1] += n
            for width in (8, 64):
                k = n // width * width
                tot[width][0] += int((~(m[:k].reshape(-1, width) == ELEV).any(1)).sum()); tot[width][1] += k // width
            # the kernel's own test: a lane cannot be elevated when it has no cell or the group's max z is under its cell's threshold + margin
            k = n // 64 * 64
            w = np.zeros(k // 8, np.float32); hg = np.zeros(9600, np.float32); cell = np.zeros(k, np.uint16)
            for which, buf in ((16, w), (10, hg), (17, cell)):
                assert c.lib.mot_debug_copy(c._h, which, b, buf.ctypes.data_as(C.c_void_p), C.c_size_t(buf.nbytes)) == 0
            with np.errstate(invalid="ignore"):
                cannot = (cell == 0xffff) | (np.repeat(w, 8).astype(np.float64) < hg[np.minimum(cell, 9599)].astype(np.float64) + MARGIN)
            assert not (cannot & (m[:k] == ELEV)).any(), "the conservative test would skip an elevated point"
            for width in (8, 64):
                cons[width][0] += int(cannot.reshape(-1, width).all(1).sum()); cons[width][1] += k // width
print(f"{a.scene} scene, {a.point_order} order, {B} streams x 2 frames of {N} points: {pts[0] / pts[1]:.3f} of the points elevated")
print(f"  8-groups (128-byte lines) without an elevated point: {tot[8][0] / tot[8][1]:.3f}")
print(f"  64-tiles (a wave's item) without an elevated point: {tot[64][0] / tot[64][1]:.3f}")
print(f"  8-groups / 64-tiles the kernel's conservative test skips: {cons[8][0] / cons[8][1]:.3f} / {cons[64][0] / cons[64][1]:.3f}")
