"""rfx.h "AOV conventions": what an engine's planes mean (world position or camera-space depth, motion in pixels or none at all, camera-space
normals) and the cameras the conversion needs — the Python form of rfx_aov_conventions, built per frame because the matrices change.
Context.set_aov_conventions hands it to the library, where the pack kernel converts on the device; imageio.aov_to_reference_conventions is the
same conversion on the host."""
from __future__ import annotations

import json
from dataclasses import dataclass, field

import numpy as np

from . import abi

DEPTH_KINDS = {"fragcoord": abi.AOV_DEPTH_FRAGCOORD, "view_z": abi.AOV_DEPTH_VIEW_Z, "position": abi.AOV_DEPTH_POSITION}
VELOCITY_KINDS = {"uv": abi.AOV_VELOCITY_UV, "scaled": abi.AOV_VELOCITY_SCALED, "cameras": abi.AOV_VELOCITY_CAMERAS}
NORMAL_SPACES = {"world": abi.AOV_NORMAL_WORLD, "view": abi.AOV_NORMAL_VIEW}
MATRICES = ("velocityMatrix", "prevVelocityMatrix", "projectionMatrix", "projectionMatrixInverse", "cameraMatrixWorld")


def _identity():
    return np.eye(4, dtype=np.float32).reshape(16)


def multiply_matrices(a, b) -> np.ndarray:
    """three.js Matrix4.multiplyMatrices(a, b) on column-major float32[16] elements, every sum in float64 in three's order
    (a_i1 b_1j + a_i2 b_2j + a_i3 b_3j + a_i4 b_4j, left to right), rounded to float32 once: what the reference uploads as
    velocityMatrix = projectionMatrix x matrixWorldInverse for an identity model matrix.  Both hosts produce these 16 floats."""
    a = [float(x) for x in np.asarray(a, np.float32).ravel()]
    b = [float(x) for x in np.asarray(b, np.float32).ravel()]
    out = np.empty(16, np.float32)
    for j in range(4):
        for i in range(4):
            s = a[i] * b[4 * j]
            s = s + a[4 + i] * b[4 * j + 1]
            s = s + a[8 + i] * b[4 * j + 2]
            s = s + a[12 + i] * b[4 * j + 3]
            out[4 * j + i] = np.float32(s)
    return out


@dataclass
class AovConventions:
    depth_kind: str = "fragcoord"      # "fragcoord" | "view_z" | "position"
    velocity_kind: str = "uv"          # "uv" | "scaled" | "cameras"
    normal_space: str = "world"        # "world" | "view"
    perspective: bool = True
    velocity_scale: tuple = (1.0, 1.0)
    near: float = 0.0
    far: float = 0.0
    velocityMatrix: np.ndarray = field(default_factory=_identity)
    prevVelocityMatrix: np.ndarray = field(default_factory=_identity)
    projectionMatrix: np.ndarray = field(default_factory=_identity)
    projectionMatrixInverse: np.ndarray = field(default_factory=_identity)
    cameraMatrixWorld: np.ndarray = field(default_factory=_identity)
    background_position: tuple | None = None  # a texel whose position equals it component-wise is not covered

    def __post_init__(self):
        if self.depth_kind not in DEPTH_KINDS or self.velocity_kind not in VELOCITY_KINDS or self.normal_space not in NORMAL_SPACES:
            raise ValueError("AOV conventions: depth_kind %s, velocity_kind %s, normal_space %s" % (sorted(DEPTH_KINDS), sorted(VELOCITY_KINDS), sorted(NORMAL_SPACES)))
        for name in MATRICES:
            m = np.asarray(getattr(self, name), np.float32).reshape(16).copy()
            setattr(self, name, m)

    @staticmethod
    def from_cameras(camera, prev_camera=None, **kinds) -> "AovConventions":
        """camera / prev_camera: anything with scene.Camera's fields (column-major float32[16] matrices, near, far, isPerspectiveCamera);
        prev_camera None: the camera did not move.  kinds: depth_kind, velocity_kind, normal_space, velocity_scale, background_position."""
        prev = prev_camera if prev_camera is not None else camera
        return AovConventions(perspective=bool(getattr(camera, "isPerspectiveCamera", True)), near=float(camera.near), far=float(camera.far),
                              velocityMatrix=multiply_matrices(camera.projectionMatrix, camera.matrixWorldInverse),
                              prevVelocityMatrix=multiply_matrices(prev.projectionMatrix, prev.matrixWorldInverse),
                              projectionMatrix=camera.projectionMatrix, projectionMatrixInverse=camera.projectionMatrixInverse,
                              cameraMatrixWorld=camera.matrixWorld, **kinds)

    @property
    def is_default(self) -> bool:
        return (self.depth_kind, self.velocity_kind, self.normal_space) == ("fragcoord", "uv", "world")

    def to_abi(self) -> abi.AovConventions:
        c = abi.AovConventions()
        c.depth_kind, c.velocity_kind, c.normal_space = DEPTH_KINDS[self.depth_kind], VELOCITY_KINDS[self.velocity_kind], NORMAL_SPACES[self.normal_space]
        c.perspective = 1 if self.perspective else 0
        c.velocity_scale[:] = [float(np.float32(x)) for x in self.velocity_scale]
        c.near_, c.far_ = float(self.near), float(self.far)
        for name in MATRICES:
            getattr(c, name)[:] = [float(x) for x in getattr(self, name)]
        c.has_background_position = 0 if self.background_position is None else 1
        if self.background_position is not None:
            c.background_position[:] = [float(np.float32(x)) for x in self.background_position]
        return c

    # the conventions record of a dump directory / a command line (--conventions JSON): every float as its exact repr
    def to_json(self) -> str:
        d = dict(depth_kind=self.depth_kind, velocity_kind=self.velocity_kind, normal_space=self.normal_space, perspective=bool(self.perspective),
                 velocity_scale=[float(x) for x in self.velocity_scale], near=float(self.near), far=float(self.far),
                 background_position=None if self.background_position is None else [float(x) for x in self.background_position])
        for name in MATRICES:
            d[name] = [float(x) for x in getattr(self, name)]
        return json.dumps(d)

    @staticmethod
    def from_json(text) -> "AovConventions":
        d = json.loads(text) if isinstance(text, (str, bytes)) else dict(text)
        if d.get("velocity_scale") is not None:
            d["velocity_scale"] = tuple(d["velocity_scale"])
        if d.get("background_position") is not None:
            d["background_position"] = tuple(d["background_position"])
        return AovConventions(**d)
