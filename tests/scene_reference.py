"""The scene detector's definition, in Python integers (docs/scene_detect.md; csrc/scene_kernels.hip must equal it bit for bit).

c_t: the model-size BGRX frame step t consumes, W x H pixels, X ignored; N = 3 W H.
S_t = sum |c_t - c_(t-1)| over the N colour bytes -- 0 while frame t-1 is not in the detector's memory.
D_t = min(S_t, |S_t - S_(t-1)|) when frames t-1 and t-2 both are in it, else 0 (ffmpeg scdet's score as a raw sum).
cut_t = (1000 D_t >= threshold_milli N).
The detector's memory starts empty (ju_create, ju_reset, a ju_set_scene_detect call that changes the mode); a detected
cut does not clear it."""

import numpy as np

OFF, REPORT, RESET = 0, 1, 2
THRESHOLD_MIN, THRESHOLD_MAX = 1, 255000
RING = 64


def problem(mode: int, threshold_milli: int) -> str:
    """The refusal of ju_set_scene_detect, "" when the pair is fine (the C layer's words)."""
    if mode not in (OFF, REPORT, RESET):
        return f"mode must be JU_SCENE_OFF (0), JU_SCENE_REPORT (1) or JU_SCENE_RESET (2), got {mode}"
    if mode != OFF and not THRESHOLD_MIN <= threshold_milli <= THRESHOLD_MAX:
        return f"threshold_milli must be 1 .. 255000, got {threshold_milli}"
    return ""


def sad(cur: np.ndarray, prev: np.ndarray) -> int:
    """S: the sum of absolute differences over B, G and R of two [H, W, 4] uint8 frames, as a Python int."""
    assert cur.shape == prev.shape and cur.dtype == np.uint8 and prev.dtype == np.uint8 and cur.shape[-1] == 4
    d = np.abs(cur[..., :3].astype(np.int16) - prev[..., :3].astype(np.int16))
    return int(d.sum(dtype=np.uint64))


def decide(s: int, s_before: int, frames_in_memory: int, n: int, threshold_milli: int):
    """(D, cut) of a step whose sum is `s`, after `frames_in_memory` frames since the start."""
    d = min(s, abs(s - s_before)) if frames_in_memory >= 2 else 0
    return d, int(1000 * d >= threshold_milli * n)


class Detector:
    """The detector of one runtime: feed it the frames the steps consume, in order."""

    def __init__(self, threshold_milli: int, step: int = 0):
        assert not problem(REPORT, threshold_milli)
        self.threshold = threshold_milli
        self.step = step            # detector steps since the mode was turned on: continues across restart()
        self.restart()

    def restart(self):
        """What ju_reset does to the detector: no predecessor."""
        self.prev, self.s_before, self.seen = None, 0, 0

    def feed(self, frame: np.ndarray) -> dict:
        frame = np.ascontiguousarray(frame)
        n = 3 * frame.shape[0] * frame.shape[1]
        s = sad(frame, self.prev) if self.seen >= 1 else 0
        d, cut = decide(s, self.s_before, self.seen, n, self.threshold)
        rec = {"step": self.step, "sad": s, "score": d, "cut": cut}
        self.prev, self.s_before = frame.copy(), s
        self.seen += 1
        self.step += 1
        return rec


def run(frames, threshold_milli: int) -> list:
    """The records of a clip fed to a fresh detector."""
    det = Detector(threshold_milli)
    return [det.feed(f) for f in frames]


def cuts(records) -> list:
    return [r["step"] for r in records if r["cut"]]


def known_clip(synthetic_frames, h: int = 30, w: int = 48) -> np.ndarray:
    """The 13-frame clip of the tests: three smooth scenes (seeds 1, 2, 3; 4, 3 and 3 frames), two all-white frames, then
    the last frame of the third scene again.  At 30 x 48 and threshold_milli 22000 the cuts are frames 4, 7, 10 and 12."""
    scenes = [synthetic_frames(n, h, w, seed=seed, kind="smooth") for seed, n in ((1, 4), (2, 3), (3, 3))]
    white = np.full((2, h, w, 4), 255, np.uint8)
    return np.concatenate(scenes + [white, scenes[2][-1:]], axis=0)


KNOWN_THRESHOLD = 22000
KNOWN_CUTS = [4, 7, 10, 12]
