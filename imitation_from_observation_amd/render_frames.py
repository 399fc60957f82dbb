"""Frames as rendered in the reward hooks (`render_size=`): the one check of what a hook is handed, the lazily made resizer and the
gather of frames into what one upload takes.  numpy only; resize.FrameResizer is imported at the first use, so a hook without
render_size never loads it."""
import numpy as np


def check_rendered(frames, size, ndim=4, what="the frames"):
    """frames as rendered are uint8 of exactly `size` + (3,): one array with `ndim` dimensions (3 a frame, 4 [n, ..], 5 [n, T, ..]),
    returned contiguous, or a list of frames, returned as a list of arrays.  TypeError for another dtype (float frames are not
    resized: imresize rescales floats by their range), ValueError for another shape -- both before anything is launched."""
    if isinstance(frames, (list, tuple)):
        return [check_rendered(f, size, 3, what) for f in frames]
    a = np.asarray(frames)
    if a.dtype != np.uint8:
        raise TypeError(f"with render_size {what} must be uint8 as rendered, got {a.dtype} (float frames are not resized)")
    want = tuple(size) + (3,)
    if a.ndim != ndim or a.shape[-3:] != want:
        lead = {5: "n, T, ", 4: "n, ", 3: ""}.get(ndim, "..., ")
        raise ValueError(f"with render_size={tuple(size)} {what} must be [{lead}{want[0]}, {want[1]}, 3], got {a.shape}")
    return np.ascontiguousarray(a)


def gather(parts, as_list=False):
    """parts: per path or video, its frames as a list or as one array [n, Hr, Wr, 3] -> what one upload takes: the flat list of
    frames, each uploaded from where it lies, or one block (a single array is handed on as it is, anything else is stacked)."""
    if as_list:
        return [f for p in parts for f in p]
    if len(parts) == 1 and isinstance(parts[0], np.ndarray):
        return parts[0]
    return np.stack([f for p in parts for f in p])


class RenderFrames:
    """What a hook with render_size holds: `size` (None without render_size), the resizer `rs` -- the injected one (anything with
    resize(); resize_u8_dev for the device chain) or a FrameResizer made at the first use from plan() -> (out_size, max_frames,
    device, stream) -- and `owned`, whether it was made here."""

    def __init__(self, render_size, plan, resizer=None):
        self.size = None if render_size is None else (int(render_size[0]), int(render_size[1]))
        self._plan, self.rs, self.owned = plan, resizer, resizer is None

    def resizer(self):
        if self.rs is None:
            from .resize import FrameResizer
            out_size, max_frames, device, stream = self._plan()
            self.rs = FrameResizer(self.size, out_size, max_frames=max_frames, device=device, stream=stream or None)
        return self.rs

    def drop(self):
        """Closes a resizer made here, so that the next use makes one from the plan as it then stands; an injected one stays."""
        if self.owned and self.rs is not None:
            self.rs.close()
            self.rs = None

    def on_device(self, consumer, *entries):
        """The device chain needs the consumer's `_dev` entries and a resizer that leaves uint8 on the device."""
        return all(hasattr(consumer, e) for e in entries) and hasattr(self.resizer(), "resize_u8_dev")

    def check(self, frames, ndim=4, what="the frames"):
        return check_rendered(frames, self.size, ndim, what)
