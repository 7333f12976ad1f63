"""Numpy float32 restatement of the RGB-D steps of the reference's Frame construction, the yardstick of the RGB-D frame
path (vsg_orb_extract_to_frame_rgbd, vsg_rgbd_depth_batch_device):

  Tracking::Tracking                 mDepthMapFactor from RGBD.DepthMapFactor            Tracking.cc:638-642
  Tracking::GrabImageRGBD            imDepth.convertTo(imDepth, CV_32F, mDepthMapFactor)  Tracking.cc:1610-1611
  Frame::ComputeStereoFromRGBD       mvDepth / mvuRight per keypoint                      Frame.cc:1129-1150

It works on the oracle's keypoints (mvKeys) and oracle_lib.undistort_keypoints (mvKeysUn).  Every operation is one
correctly rounded float32 operation, as in an SSE2 build of the reference: convertTo's cvt_32f is x * scale + 0
([OCV 4.2]), the division and the subtraction are not contracted.  Keypoints whose truncated pixel lies outside the
plane, or whose coordinates are NaN, get -1 / -1: the reference reads out of bounds there (undefined behaviour), the
library must not."""
import numpy as np

F32 = np.float32


def depth_map_scale(yaml_value):
    """mDepthMapFactor: fabs(yaml) < 1e-5 -> 1, otherwise 1.0f / yaml (Tracking.cc:638-642)."""
    v = F32(yaml_value)
    if float(abs(v)) < 1e-5:
        return F32(1.0)
    return F32(F32(1.0) / v)


def needs_conversion(dtype, scale):
    """if((fabs(mDepthMapFactor-1.0f)>1e-5) || imDepth.type()!=CV_32F): the difference in float, the compare in double."""
    return float(abs(F32(F32(scale) - F32(1.0)))) > 1e-5 or np.dtype(dtype) != np.float32


def convert_depth(depth, scale):
    """The CV_32F plane Frame::ComputeStereoFromRGBD reads (uint16 or float32 input)."""
    d = np.asarray(depth)
    if d.dtype not in (np.uint16, np.float32):
        raise TypeError("depth planes are uint16 or float32")
    if not needs_conversion(d.dtype, scale):
        return d.astype(np.float32, copy=True)  # read unscaled
    with np.errstate(all="ignore"):
        return (d.astype(np.float32) * F32(scale)).astype(np.float32)


def compute_stereo_from_rgbd(keys, keys_un, depth32, mbf):
    """(mvuRight, mvDepth) of Frame::ComputeStereoFromRGBD: d = imDepth.at<float>((int)kp.pt.y, (int)kp.pt.x) with
    kp = mvKeys[i]; d > 0 -> {kpU.pt.x - mbf / d, d}, otherwise {-1, -1}."""
    x = np.ascontiguousarray(keys["x"], dtype=np.float32)
    y = np.ascontiguousarray(keys["y"], dtype=np.float32)
    xu = np.ascontiguousarray(keys_un["x"], dtype=np.float32)
    rows, cols = depth32.shape
    with np.errstate(invalid="ignore"):
        inside = (x > F32(-1)) & (y > F32(-1)) & (x < F32(cols)) & (y < F32(rows))  # NaN: False
    col = np.where(inside, x, F32(0)).astype(np.int32)  # float -> int truncates toward zero, like (int)
    row = np.where(inside, y, F32(0)).astype(np.int32)
    d = np.where(inside, depth32[row, col], F32(-1)).astype(np.float32)
    with np.errstate(all="ignore"):
        pos = d > F32(0)
        ur = (xu - F32(mbf) / np.where(pos, d, F32(1))).astype(np.float32)
    u_right = np.where(pos, ur, F32(-1)).astype(np.float32)
    depth = np.where(pos, d, F32(-1)).astype(np.float32)
    return u_right, depth


def rgbd_frame(keys, keys_un, depth, scale, mbf):
    """Both steps: the raw plane (uint16 / float32) and mDepthMapFactor in, (mvuRight, mvDepth) out."""
    return compute_stereo_from_rgbd(keys, keys_un, convert_depth(depth, scale), mbf)


def depth_plane(seed, rows, cols, dtype, holes=0.1):
    """A seeded depth plane with holes (0) -- what a RealSense / TUM PNG delivers: uint16 millimetre-like values, or the
    same in metres as float32."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:rows, 0:cols]
    base = 800 + 3000 * (0.5 + 0.5 * np.sin(xx / 37.0 + seed) * np.cos(yy / 23.0))
    d = (base + rng.integers(0, 200, (rows, cols))).astype(np.uint16)
    d[rng.random((rows, cols)) < holes] = 0
    if np.dtype(dtype) == np.float32:
        return (d.astype(np.float32) * F32(0.001)).astype(np.float32)
    return d
