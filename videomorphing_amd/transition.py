"""Schedule builders for transition control (vm_frame_upload_schedule, morph.Frame.upload_schedule).
Host only, numpy only.  A schedule is an (h, w, 2) float32 plane of pairs (t0, t1) in the halfway domain: the texel
starts its transition at time t0 and ends it at t1.  Every builder spreads the starts over [0, lead] and gives every
texel the same duration, so with lead + duration == 1 the whole transition runs from t = 0 to t = 1."""
import numpy as np


def _schedule(start, duration):
    s = np.empty(start.shape + (2,), np.float32)
    s[..., 0] = start
    s[..., 1] = start + float(duration)
    return s


def uniform(w, h, t0=0.0, t1=1.0):
    """every texel (t0, t1): (0, 1) is the schedule under which a transition call equals its uniform counterpart"""
    s = np.empty((int(h), int(w), 2), np.float32)
    s[..., 0], s[..., 1] = t0, t1
    return s


def wipe(w, h, direction=(1.0, 0.0), lead=0.6, duration=0.4):
    """a linear wipe along `direction` (dx, dy; need not be normalised): the texel the direction meets first starts at
    0, the last one at `lead`; duration 0 is a hard edge"""
    dx, dy = float(direction[0]), float(direction[1])
    assert dx != 0.0 or dy != 0.0
    y, x = np.mgrid[0:int(h), 0:int(w)].astype(np.float64)
    p = x * dx + y * dy
    span = p.max() - p.min()
    pos = (p - p.min()) / span if span > 0 else np.zeros_like(p)
    return _schedule(float(lead) * pos, duration)


def radial(w, h, centre=None, lead=0.6, duration=0.4):
    """from `centre` (x, y in pixels; default: the middle of the frame) outwards: the centre starts at 0, the farthest
    texel at `lead`"""
    cx, cy = ((int(w) - 1) / 2.0, (int(h) - 1) / 2.0) if centre is None else (float(centre[0]), float(centre[1]))
    y, x = np.mgrid[0:int(h), 0:int(w)].astype(np.float64)
    r = np.hypot(x - cx, y - cy)
    return _schedule(float(lead) * (r / r.max() if r.max() > 0 else r), duration)


def from_matte(matte, lead=0.5, duration=None):
    """a matte in [0, 1] over the halfway domain: the foreground (1) starts at 0, the background (0) `lead` later, what
    lies between in proportion; duration defaults to 1 - lead"""
    m = np.clip(np.asarray(matte, dtype=np.float64), 0.0, 1.0)
    assert m.ndim == 2
    return _schedule(float(lead) * (1.0 - m), 1.0 - float(lead) if duration is None else duration)
