"""Rendering of environment states: cameras resolved into dm_render_desc, image tiling, frame files.

The images come from dm_batch_render (csrc/render_kernel.h); this module only describes the scene and the camera.  Two
camera kinds map onto the descriptor's one form (a position in the world or relative to the centre of mass, a 3x3 frame
whose columns are the camera's x, y, z axes, and a vertical field of view):

  * a model camera by name (`humanoid_visual()["cameras"]`, dp_env_v3.xml:23-24): trackcom cameras keep their offset from
    the centre of mass and their world orientation at qpos0;
  * a `FreeCamera` (MuJoCo's mjvCamera: lookat, distance, azimuth, elevation in degrees), optionally tracking the COM.
"""
import math
import os

import numpy as np

from . import _abi as A
from .humanoid import DEFAULT_FOVY, humanoid_visual

DEFAULT_CAMERA = "side"


class FreeCamera(object):
    """mjvCamera angles: forward f = (cos el cos az, cos el sin az, sin el), position = lookat - distance f, x = f x (0, 0, 1)
    normalised, y = x x f, z = -f.  track_com: lookat is an offset from the centre of mass of each rendered state."""

    def __init__(self, lookat=(0.0, 0.0, 1.0), distance=4.0, azimuth=90.0, elevation=-20.0, track_com=False, fovy=DEFAULT_FOVY):
        self.lookat = tuple(float(v) for v in lookat)
        self.distance, self.azimuth, self.elevation = float(distance), float(azimuth), float(elevation)
        self.track_com, self.fovy = bool(track_com), float(fovy)

    def frame(self):
        """-> (position [3], row-major frame [9])"""
        az, el = math.radians(self.azimuth), math.radians(self.elevation)
        f = np.array([math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el)])
        x = np.cross(f, [0.0, 0.0, 1.0])
        if np.linalg.norm(x) < 1e-9:
            raise ValueError("a free camera cannot look straight up or down")
        x /= np.linalg.norm(x)
        y = np.cross(x, f)
        pos = np.asarray(self.lookat) - self.distance * f
        return pos, np.column_stack([x, y, -f]).reshape(9)


def subtree_com(cm, xipos):
    """centre of mass of the root's subtree: sum m xipos / sum m over bodies 1..nbody-1"""
    m = np.asarray(cm.body_mass[1:], dtype=np.float64)
    return (m[:, None] * np.asarray(xipos)[1:]).sum(0) / m.sum()


def camera_frame(xyaxes):
    """MJCF xyaxes -> row-major frame: x normalised, y Gram-Schmidt against x, z = x cross y"""
    x = np.asarray(xyaxes[:3], dtype=np.float64); y = np.asarray(xyaxes[3:], dtype=np.float64)
    x = x / np.linalg.norm(x)
    y = y - (y @ x) * x
    y = y / np.linalg.norm(y)
    return np.column_stack([x, y, np.cross(x, y)]).reshape(9)


def resolve_camera(cm, camera=DEFAULT_CAMERA, visual=None):
    """-> (pos [3], mat [9], fovy degrees, track_com) for a model camera's name or a FreeCamera"""
    if isinstance(camera, FreeCamera):
        pos, mat = camera.frame()
        return pos, mat, camera.fovy, camera.track_com
    visual = visual or humanoid_visual()
    cams = {c["name"]: c for c in visual["cameras"]}
    if camera not in cams:
        raise ValueError("unknown camera %r (the model has %s)" % (camera, sorted(cams)))
    c = cams[camera]
    xpos, xmat, xipos = cm.kinematics(cm.qpos0)[:3]
    b = int(c["body"])
    local = camera_frame(c["xyaxes"]).reshape(3, 3)
    pos = xpos[b] + xmat[b] @ np.asarray(c["pos"], dtype=np.float64)
    mat = (xmat[b] @ local).reshape(9)
    if c["mode"] == "trackcom":
        return pos - subtree_com(cm, xipos), mat, float(c["fovy"]), True
    if c["mode"] == "fixed" and b == 0:
        return pos, mat, float(c["fovy"]), False
    raise ValueError("camera %r: mode %r on body %d is not supported (trackcom, or fixed in the world body)" % (camera, c["mode"], b))


def make_desc(cm, width, height, camera=DEFAULT_CAMERA, visual=None):
    """the dm_render_desc of one call: image size, the resolved camera, and the scene's colours and light from `visual`"""
    visual = visual or humanoid_visual()
    d = A.RenderDesc()
    d.width, d.height = int(width), int(height)
    pos, mat, fovy, track = resolve_camera(cm, camera, visual)
    d.track_com = 1 if track else 0
    for k in range(3):
        d.cam_pos[k] = float(pos[k])
    for k in range(9):
        d.cam_mat[k] = float(mat[k])
    d.fovy = float(fovy)
    for g in range(A.NGEOM):
        for k in range(3):
            d.geom_rgb[g][k] = float(visual["geom_rgba"][k])
    fl = visual["floor"]
    # a builtin checker is 2 x 2 squares per texture repeat: with texuniform one repeat per metre, else one across the plane
    extent = 1.0 if fl["texuniform"] else 2.0 * float(cm.geom_size[fl["geom"]][0])
    d.floor_square = extent / (2.0 * float(fl["texrepeat"][0]))
    sky, light = visual["skybox"], visual["light"]
    for k in range(3):
        d.floor_rgb1[k], d.floor_rgb2[k] = float(fl["rgb1"][k]), float(fl["rgb2"][k])
        d.sky_top[k], d.sky_bottom[k] = float(sky["rgb1"][k]), float(sky["rgb2"][k])
        d.light_dir[k] = float(light["dir"][k])
    d.ambient, d.headlight = float(visual["headlight"]["ambient"]), float(visual["headlight"]["diffuse"])
    d.diffuse = float(light["diffuse"][0])
    return d


def tile_images(img_nhwc):
    """N images [N, h, w, c] -> one image of ceil(sqrt(N)) rows of tiles, filled row by row and padded with black
    (OpenAI baselines' vec_env.tile_images)."""
    img_nhwc = np.asarray(img_nhwc)
    N, h, w, c = img_nhwc.shape
    H = int(np.ceil(np.sqrt(N)))
    W = int(np.ceil(float(N) / H))
    img_nhwc = np.array(list(img_nhwc) + [img_nhwc[0] * 0 for _ in range(N, H * W)])
    return img_nhwc.reshape(H, W, h, w, c).transpose(0, 2, 1, 3, 4).reshape(H * h, W * w, c)


class FrameWriter(object):
    """Collects uint8 frames [H, W, 3] and writes them on close(): an animated GIF through PIL when it imports and the path
    ends in .gif, otherwise an .npy array [T, H, W, 3] next to it.  close() returns the path written."""

    def __init__(self, path, fps=30):
        self.path, self.fps, self.frames = path, float(fps), []

    def add(self, frame):
        f = np.asarray(frame)
        if f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 3:
            raise ValueError("a frame is uint8 [H, W, 3]")
        self.frames.append(f.copy())

    def close(self):
        if not self.frames:
            raise ValueError("no frames to write")
        d = os.path.dirname(os.path.abspath(self.path))
        os.makedirs(d, exist_ok=True)
        try:
            from PIL import Image
        except ImportError:
            Image = None
        if Image is not None and self.path.lower().endswith(".gif"):
            imgs = [Image.fromarray(f) for f in self.frames]
            imgs[0].save(self.path, save_all=True, append_images=imgs[1:], duration=max(1, int(round(1000.0 / self.fps))), loop=0)
            return self.path
        out = self.path if self.path.endswith(".npy") else os.path.splitext(self.path)[0] + ".npy"
        np.save(out, np.stack(self.frames))
        return out


def write_frames(path, frames, fps=30):
    w = FrameWriter(path, fps)
    for f in frames:
        w.add(f)
    return w.close()


def read_frames(path):
    """frames written by FrameWriter -> uint8 [T, H, W, 3]"""
    if path.endswith(".npy"):
        return np.load(path)
    from PIL import Image, ImageSequence
    with Image.open(path) as im:
        return np.stack([np.asarray(f.convert("RGB")) for f in ImageSequence.Iterator(im)])
