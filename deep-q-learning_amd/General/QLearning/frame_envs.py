"""Pixel vector envs for the CNN agent (CnnVectorAgent(env=...)), and Catch, a deterministic toy one.

The protocol. A pixel vector env is any object with
  n_envs                 the number of envs n
  A (optional)           the number of actions; CnnVectorAgent checks it against its num_actions
  reset()                -> frames u8 [n, F, H, W, C]: the first images of n new episodes
  step(actions int32[n]) -> (frames u8 [n, F, H, W, C], rewards f32 [n], dones bool [n], reset_frames u8 [k, F, H, W, C])
where
  frames        the images of the step (for an env whose episode just ended: its last images); F in {1, 2} are the last raw
                frames of a frame-skip step (the device takes their max), C in {3, 1} is RGB or gray; 84 <= H, W <= 512. The F
                axis may be left out when F = 1 and the C axis when C = 1.
  dones         the episode ended, by termination or by truncation (what the replay ring stores as d, q_agent.py:179-180)
  reset_frames  the first images of the new episodes of the envs that reset themselves, in ascending env order: exactly the
                done ones, so k == dones.sum()
The env runs on the host (or anywhere); its images go to the device as they are, and the device does the rest -- luma, the max
over F, the area resize to 84 x 84, the four-frame stacks, the replay ring (CnnEngine.env_observe, one launch per step).

A gymnasium Atari vector env fits after a thin wrapper (documentation only): make the envs with
frameskip=1 and no preprocessing wrapper, repeat each action 4 times inside step() keeping the last two raw RGB frames
(F = 2, C = 3, 210 x 160, or obs_type="grayscale" for C = 1), and reset the done envs within the same step (same-step
autoreset, or an explicit reset of those envs): their first frames go into reset_frames.
"""
from __future__ import annotations

import numpy as np


def reset_slots(dones, reset_frames, n_envs):
    """the reset_slot input of CnnEngine.env_observe: row of reset_frames for each done env (ascending), -1 elsewhere. Raises
    ValueError unless dones is [n] and reset_frames holds exactly dones.sum() images"""
    d = np.asarray(dones)
    if d.shape != (n_envs,):
        raise ValueError(f"dones must have shape ({n_envs},), got {d.shape}")
    d = d.astype(bool)
    k = int(d.sum())
    m = 0 if reset_frames is None else int(np.shape(reset_frames)[0])
    if m != k:
        raise ValueError(f"{k} envs are done but reset_frames holds {m} images")
    slot = np.full(n_envs, -1, np.int32)
    slot[d] = np.arange(k, dtype=np.int32)
    return slot


class Catch:
    """Catch as a pixel vector env: a 5 x 10 grid of 32 x 19-pixel cells under a 20-pixel top margin (210 x 160 images). A ball
    falls one row per step from a random column of the top row; the one-cell paddle on the bottom row moves left / stays / right
    (actions 0, 1, 2). When the ball reaches the bottom row (after 9 steps) the episode ends with reward +1 if the paddle is under
    it and -1 otherwise, and the env starts a new one.

    frames=2 (default) emits the last two raw frames of a step with flicker: the ball is drawn in only one of them, alternating by
    step, so without the max over the two frames it vanishes from half the preprocessed images. channels=3 (default) emits RGB
    on a non-black background, channels=1 the luma of the same colours. Deterministic for a seed."""
    ROWS, COLS, CELL_H, CELL_W, TOP = 10, 5, 19, 32, 20
    H, W, A = 210, 160, 3
    RGB = {"bg": (40, 80, 140), "ball": (250, 220, 40), "paddle": (220, 40, 200)}

    def __init__(self, n_envs, seed=0, frames=2, channels=3):
        if frames not in (1, 2) or channels not in (1, 3):
            raise ValueError("Catch: frames must be 1 or 2, channels 1 or 3")
        self.n_envs, self.F, self.C = int(n_envs), int(frames), int(channels)
        self.rng = np.random.default_rng(seed)
        col = lambda rgb: np.array(rgb if channels == 3 else [(4899 * rgb[0] + 9617 * rgb[1] + 1868 * rgb[2] + 8192) >> 14], np.uint8)
        self.bg, self.ball_c, self.paddle_c = col(self.RGB["bg"]), col(self.RGB["ball"]), col(self.RGB["paddle"])
        n = self.n_envs
        self.ball_row, self.ball_col = np.zeros(n, np.int64), np.zeros(n, np.int64)
        self.paddle, self.t = np.zeros(n, np.int64), np.zeros(n, np.int64)

    def _new_episodes(self, envs):
        self.ball_row[envs] = 0
        self.ball_col[envs] = self.rng.integers(0, self.COLS, len(envs))
        self.paddle[envs] = self.COLS // 2
        self.t[envs] = 0

    def _cells(self, out, frame, rows, cols, colour):
        """paint cell (rows[k], cols[k]) of frame frame[k] of image k"""
        k = np.arange(len(rows))
        y = self.TOP + rows[:, None] * self.CELL_H + np.arange(self.CELL_H)
        x = cols[:, None] * self.CELL_W + np.arange(self.CELL_W)
        out[k[:, None, None], frame[:, None, None], y[:, :, None], x[:, None, :]] = colour

    def render(self, envs):
        """images u8 [len(envs), F, 210, 160, C] of the envs' current states"""
        k = len(envs)
        out = np.empty((k, self.F, self.H, self.W, self.C), np.uint8)
        out[...] = self.bg
        for f in range(self.F):
            self._cells(out, np.full(k, f), np.full(k, self.ROWS - 1), self.paddle[envs], self.paddle_c)
        ball_frame = self.t[envs] % 2 if self.F == 2 else np.zeros(k, np.int64)     # flicker: one of the two raw frames
        self._cells(out, ball_frame, self.ball_row[envs], self.ball_col[envs], self.ball_c)
        return out

    def reset(self):
        envs = np.arange(self.n_envs)
        self._new_episodes(envs)
        return self.render(envs)

    def step(self, actions):
        a = np.asarray(actions).astype(np.int64)
        if a.shape != (self.n_envs,) or a.min() < 0 or a.max() >= self.A:
            raise ValueError(f"Catch.step: actions must be int [{self.n_envs}] in [0, {self.A})")
        self.paddle = np.clip(self.paddle + a - 1, 0, self.COLS - 1)
        self.ball_row += 1
        self.t += 1
        dones = self.ball_row == self.ROWS - 1
        rewards = np.where(dones, np.where(self.paddle == self.ball_col, 1.0, -1.0), 0.0).astype(np.float32)
        frames = self.render(np.arange(self.n_envs))
        done_envs = np.flatnonzero(dones)
        self._new_episodes(done_envs)
        return frames, rewards, dones, self.render(done_envs)
