"""gsaj -- torch-tensor front end of libgsaj_hip.so.  Submodules are imported by name (gsaj.rasterizer, gsaj.tracking, ...);
the package itself imports nothing, so that `from gsaj import synthetic` needs neither torch nor the library."""
__all__ = ["GaussNewtonTracker", "GaussNewtonWindow", "PyramidGaussNewtonTracker", "StereoMatcher", "StereoIngest", "RgbdAligner",
           "JointRgbdAligner", "MotionStereo", "grey_u8"]


def __getattr__(name):
    if name == "GaussNewtonTracker":  # gsaj.GaussNewtonTracker: second-order tracking (gsaj.gauss_newton), loaded on first use
        from .gauss_newton import GaussNewtonTracker
        return GaussNewtonTracker
    if name == "GaussNewtonWindow":   # K such solves against one fixed map in one set of launches
        from .gauss_newton import GaussNewtonWindow
        return GaussNewtonWindow
    if name == "PyramidGaussNewtonTracker":  # one such solve coarse to fine over a device image pyramid
        from .gauss_newton import PyramidGaussNewtonTracker
        return PyramidGaussNewtonTracker
    if name in ("StereoMatcher", "StereoIngest"):  # a stereo pair to disparity, depth and the left colour (gsaj.stereo)
        from . import stereo
        return getattr(stereo, name)
    if name in ("RgbdAligner", "JointRgbdAligner"):  # the start pose of a new frame from the last tracked frame alone (gsaj.align);
        from . import align                           # Joint: its brightness change against that frame solved with the pose
        return getattr(align, name)
    if name in ("MotionStereo", "grey_u8"):  # the depth of a monocular keyframe from a second frame and the two tracked poses
        from . import motion_stereo               # (gsaj.motion_stereo); grey_u8: a tracker's colour as that matcher's input bytes
        return getattr(motion_stereo, name)
    raise AttributeError("module 'gsaj' has no attribute %r" % name)
