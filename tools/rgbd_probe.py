"""Kernel-time probe of the RGB-D frame path, meant to run under  rocprofv3 --kernel-trace --stats  (profiles/README.md):

  batch  k_rgbd_batch at B frames of C2 geometry (640x480, capacity of 1000 features) with the TUM1 camera's distortion,
         on synthetic records spread over the image (every record valid); prints the byte count the kernel must move
  grid   vsg_orb_extract_to_frame (gray only) N times, then vsg_orb_extract_to_frame_rgbd N times (pinned uint16 depth), at
         640x480 / 1250 features with the TUM1 camera: k_frame_grid_build's dispatches split in two halves

usage: python3 tools/rgbd_probe.py {batch B reps | grid N}"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import torch  # noqa: E402  (torch's HIP runtime first, as in tests/conftest.py)

import oracle_lib as ol  # noqa: E402
import rgbd_reference as rr  # noqa: E402
from visual_sgraphs_amd import orb, synth  # noqa: E402

W, H = 640, 480


def batch(B, reps):
    cam = ol.scaled_camera("tum1", W, H)
    cap = 1024
    rng = np.random.default_rng(1)
    k = np.zeros((B, cap), orb.KP_DTYPE)
    k["x"], k["y"] = rng.uniform(0, W, (B, cap)), rng.uniform(0, H, (B, cap))
    dev = torch.device("cuda", 0)
    d_k = torch.from_numpy(k.view(np.uint8).reshape(B, cap, 28)).to(dev)
    d_c = torch.from_numpy(np.tile(np.array([[cap, 0]], np.int32), (B, 1))).to(dev)
    plane = rr.depth_plane(5, H, W, np.uint16)
    d_p = torch.from_numpy(np.tile(plane.view(np.int16)[None], (B, 1, 1))).to(dev)
    d_ur = torch.empty((B, cap), dtype=torch.float32, device=dev)
    d_dp = torch.empty((B, cap), dtype=torch.float32, device=dev)
    for _ in range(reps):
        orb.rgbd_depth_batch_device(d_p.data_ptr(), orb.VSG_DEPTH_U16, B, H * W * 2, W * 2, H, W, np.float32(0.0002),
                                    np.float32(40.0), cam["K4"], cam["dist"], d_k.data_ptr(), d_c.data_ptr(), cap,
                                    d_ur.data_ptr(), d_dp.data_ptr(), None)
    torch.cuda.synchronize(dev)
    recs = B * cap
    # the bytes the launch must move: each record read (28 B), two floats written (8 B), and the one depth pixel it reads,
    # which costs a whole 128-byte line (gfx950's L2 request size): the random positions rarely share a line, so this
    # counts one line per record -- an estimate, not a measurement
    line_bytes = recs * 128
    print({"B": B, "records": recs, "record_bytes": recs * 36, "depth_line_bytes": line_bytes,
           "bytes": recs * 36 + line_bytes, "bound_us_at_8TBps": (recs * 36 + line_bytes) / 8e12 * 1e6})


def grid(N):
    cam = ol.scaled_camera("tum1", W, H)
    bounds = ol.image_bounds(cam)
    ex = orb.ORBextractor(1250, 1.2, 8, 20, 7)
    f = orb.Frame(ex.capacity(H, W))
    img = synth.sequence_frame(W, H, 5, 0)
    pinned = orb.PinnedArray((H, W), np.uint16)
    pinned.a[:] = rr.depth_plane(5, H, W, np.uint16)
    for _ in range(N):
        f.extract_into(ex, img, bounds, cam["K4"], cam["dist"])
    for _ in range(N):
        r = f.extract_into_rgbd(ex, img, pinned.a, bounds, cam["K4"], cam["dist"], np.float32(0.0002), np.float32(40.0))
    print({"N": N, "features": len(r[1]), "with_depth": int(np.sum(r[4] > 0))})


if __name__ == "__main__":
    if sys.argv[1] == "batch":
        batch(int(sys.argv[2]), int(sys.argv[3]))
    else:
        grid(int(sys.argv[2]))
