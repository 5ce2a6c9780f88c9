"""Drop-in for the `apriltag` Python module the reference imports.

The reference does `from apriltag import apriltag`, constructs `apriltag(tag_type)` and
calls `.detect(gray)` (reference src/detection/tag_detector.py:11,18,26).  Upstream's module
is a CPython extension around the AprilRobotics C detector; this shim has the same
constructor keywords and result shape, and forwards to the HIP detector through the C ABI
(include/aprilslam.h: asl_detector_create / asl_detect_gray_u8).  There is no CPU path.

`lib/apriltag/build/apriltag.py` re-exports this module from the location the reference
puts on sys.path (tag_detector.py:7-9).
"""
import numpy as np

from . import _lib


class apriltag(object):
    def __init__(self, family, threads=1, maxhamming=1, decimate=2.0, blur=0.0, refine_edges=True, debug=False,
                 device=0, id_limit=None):
        """family: a name, or a list / tuple of registered names for one detector that decodes them all in one pass.
        With a list the detections' 'id' is global (family i's ids follow those of the families before it) and they carry
        two more keys, 'family' (the name) and 'local_id'."""
        many = isinstance(family, (list, tuple))
        if not (all(isinstance(f, str) for f in family) if many else isinstance(family, str)):
            raise TypeError("family must be a string or a list of strings")
        if many and id_limit is not None:
            raise RuntimeError("id_limit is for one family")
        try:
            # id_limit=None: only the ids the reference pins (0..4) are decoded; 0 opens the build-defined rest
            # blur (upstream's quad_sigma) goes in through the setter: asl_detector_create itself takes 0 only
            self._det = _lib.Detector(list(family) if many else family, threads, maxhamming, decimate, 0.0, refine_edges, device, id_limit)
            if blur != 0:
                self._det.set_quad_sigma(blur)
        except _lib.AslError as e:
            # upstream raises RuntimeError for an unrecognised family / bad options
            raise RuntimeError(str(e))
        self.family = tuple(family) if many else family
        self.debug = bool(debug)

    def family_keys(self, tag_id):
        """The keys a detection of a several-family detector carries on top of upstream's: {} for one family."""
        if isinstance(self.family, str):
            return {}
        index, local_id = self._det.family_of(tag_id)
        return {"family": self.family[index], "local_id": local_id}

    def detect(self, image):
        """image: 2-D uint8 array.  Returns a tuple of dicts with the keys upstream's wrapper
        emits: 'hamming', 'margin', 'id', 'center', 'lb-rb-rt-lt' (and 'family', 'local_id' for a list of families)."""
        a = np.asarray(image)
        if a.ndim != 2 or a.dtype != np.uint8:
            raise RuntimeError("Expected a 2-D uint8 array (got ndim=%d dtype=%s)" % (a.ndim, a.dtype))
        dets, _ = self._det.detect_host(np.ascontiguousarray(a))
        return tuple(
            dict({"hamming": int(d["hamming"]), "margin": float(d["margin"]), "id": int(d["id"]),
                  "center": np.array(d["center"], dtype=np.float64), "lb-rb-rt-lt": np.array(d["corners"], dtype=np.float64)},
                 **self.family_keys(int(d["id"])))
            for d in dets)
