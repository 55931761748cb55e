"""Dataset side of the train scripts: the callers and data formats just before the hot path
(SURVEY.md 8(f) row 4). Same names, arguments and results as the reference's utils.py:15-194 and the
split / sampler block of phase3/train.py:114-162, so that `phase*/train*.py` run on a
*Music-to-Dance-Motion-Synthesis* folder as well as on `--synthetic` batches.

What differs from the reference, on purpose:
  * MinMax scaling is a small class of our own (`MinMaxScaler`, the subset of sklearn's the reference uses:
    fit / transform / fit_transform / inverse_transform with `data_min_`, `data_max_`, `scale_`, `min_`), with a
    device form (`transform_device` / `inverse_transform_device`: one HIP kernel, m2d_affine_cols) for tensors
    that already live in HBM - the sampling paths of phase2/train.py:192-193 and phase3/test.py:92-101;
  * wav files are read with scipy.io.wavfile (librosa is not a dependency): 16-bit / 32-bit PCM is scaled to
    [-1, 1) and multi-channel audio averaged, which is what `librosa.load(path, sr=None)` returns for them;
  * the takes of a dataset are stored columnar (one array + offsets, `_Ragged`); `collate_fn(..., device=)` pads with
    one masked gather, on the device when asked (default: host tensors, as the reference returns them), and
    `SequenceDataset.sample_batch(indices, device=)` cuts a whole batch of windows out of the HBM-resident store;
  * `SequenceDataset(crop_rng=)`: an explicit generator for the window starts (default: numpy's global one, as in the
    reference); `make_loaders` returns no validation loader when the hold-out is empty;
  * `SequenceDataset(augment=)` / the YAML's `dataset: augment:` (off by default): training windows under a drawn
    playback speed, mirror, yaw and audio gain - the rule is `augment_window` (host, fp64), the resident gather applies
    it in one HIP launch (m2d_crop_augment). The reference augments on disk (augment_data.py: mirrored waltz copies).
Nothing here is on the timed path; the kernels it calls are declared in include/m2d.h.
"""
import collections
import json
import math
import os
import pickle

import numpy as np
import torch
from torch.utils.data import Dataset

from . import kernels


# --------------------------------------------------------------------------------------- MinMax scaling
class MinMaxScaler:
    """sklearn.preprocessing.MinMaxScaler(feature_range=(0, 1)) as the reference uses it (utils.py:26-31,79-85):
    per-feature `scale_ = 1 / (max - min)` (1 where max == min), `min_ = -min * scale_`; transform X * scale_ + min_."""

    def __init__(self):
        self.data_min_ = self.data_max_ = self.data_range_ = self.scale_ = self.min_ = None
        self._dev = {}

    def fit(self, X):
        X = np.asarray(X, dtype=np.float64)
        self.data_min_ = X.min(axis=0)
        self.data_max_ = X.max(axis=0)
        self.data_range_ = self.data_max_ - self.data_min_
        rng = self.data_range_.copy()
        rng[rng < 10 * np.finfo(rng.dtype).eps] = 1.0  # sklearn's _handle_zeros_in_scale: constant features keep scale 1
        self.scale_ = 1.0 / rng
        self.min_ = 0.0 - self.data_min_ * self.scale_
        self.n_features_in_ = X.shape[1]
        self._dev = {}
        return self

    def transform(self, X):
        X = np.array(X, dtype=np.float64, copy=True)
        X *= self.scale_
        X += self.min_
        return X

    def fit_transform(self, X):
        return self.fit(X).transform(X)

    def inverse_transform(self, X):
        X = np.array(X, dtype=np.float64, copy=True)
        X -= self.min_
        X /= self.scale_
        return X

    # device forms: (..., n_features) fp32 tensors in HBM, one kernel each
    def _coeffs(self, device, inverse):
        key = (str(device), inverse)
        c = self._dev.get(key)
        if c is None:
            if inverse:
                a, b = 1.0 / self.scale_, -self.min_ / self.scale_
            else:
                a, b = self.scale_, self.min_
            c = self._dev[key] = (torch.as_tensor(a, dtype=torch.float32).to(device),
                                  torch.as_tensor(b, dtype=torch.float32).to(device))
        return c

    def transform_device(self, x, out=None):
        a, b = self._coeffs(x.device, False)
        return kernels.impl().affine_cols(x.contiguous(), a, b, out)

    def inverse_transform_device(self, x, out=None):
        a, b = self._coeffs(x.device, True)
        return kernels.impl().affine_cols(x.contiguous(), a, b, out)


# --------------------------------------------------------------------------------------- file loaders
def _read_wav(path):
    """librosa.load(path, sr=None) for PCM / float wav files: float32 mono in [-1, 1)."""
    from scipy.io import wavfile
    _, data = wavfile.read(path)
    if data.dtype == np.int16:
        data = data.astype(np.float32) / 32768.0
    elif data.dtype == np.int32:
        data = data.astype(np.float32) / 2147483648.0
    elif data.dtype == np.uint8:
        data = (data.astype(np.float32) - 128.0) / 128.0
    else:
        data = data.astype(np.float32)
    if data.ndim > 1:
        data = data.mean(axis=1)
    return data


def _dance_dirs(name):
    for directory in os.listdir("{}".format(name)):
        directory = "{}/{}".format(name, directory)
        base = os.path.basename(directory)
        if os.path.isdir(directory) and base[0:5] == "DANCE" and base[-3:] != "bis":
            yield directory, base


def _skeleton_file(base):
    return "/new_skeletons.json" if base[6] == "W" else "/skeletons.json"


def load_sticks(name):
    """utils.py:147-162: the skeleton JSON of every DANCE_* folder (waltz folders use new_skeletons.json)."""
    sticks = []
    for directory, base in _dance_dirs(name):
        file = _skeleton_file(base)
        if os.path.exists(directory + file):
            with open(directory + file) as f:
                sticks.append(json.load(f))
    return sticks


SYNC_FILE = "sync.json"


def sync_heads(lag_frames, hop):
    """What an estimated lag removes at the head of a take -> (pose frames, audio samples): lag l > 0, the motion lags
    the audio by l frames - the first l pose frames go; l < 0 - the first -l hop audio samples go. Frame 0 and
    sample 0 of what is left belong together."""
    l = int(lag_frames)
    return (l, 0) if l > 0 else (0, -l * int(hop))


def read_sync(directory):
    """The take's sync.json (prepare_data --sync) when it exists, is accepted and names a lag; else None"""
    path = os.path.join(directory, SYNC_FILE)
    if not os.path.exists(path):
        return None
    with open(path) as f:
        est = json.load(f)
    return est if est.get("accepted") and est.get("lag_frames") is not None else None


def apply_sync(take, music, est):
    """-> (take, music) with the heads sync_heads(est) names removed ('skeletons', 'center' and 'length' of the take)"""
    frames, samples = sync_heads(est["lag_frames"], est["hop"])
    if frames:
        take = dict(take)
        for key in ("skeletons", "center"):
            if key in take:
                take[key] = take[key][frames:]
        if "length" in take:
            take["length"] = len(take["skeletons"])
    return take, music[samples:]


def load_all(name, dance_types, augment=False, sync=False):
    """utils.py:165-194: skeleton JSONs, resampled audio tracks, style letters and folder names. sync (extension): a
    take whose folder holds an accepted sync.json is trimmed at its head (apply_sync); the others are left as they are."""
    sticks, musics, labels, dirs = [], [], [], []
    for directory, base in _dance_dirs(name):
        if base[6] not in dance_types:
            continue
        dirs.append(directory)
        labels.append(base[6])
        music = _read_wav(directory + "/resampled_audio_extract.wav")
        with open(directory + _skeleton_file(base)) as f:
            take = json.load(f)
        est = read_sync(directory) if sync else None
        if est is not None:
            take, music = apply_sync(take, music, est)
        musics.append(music)
        sticks.append(take)
    return sticks, musics, labels, dirs


def stickwise(dataset, attribute):
    """utils.py:196-201: all frames of all sequences, concatenated ('skeletons' | 'center')."""
    return np.concatenate([np.asarray(seq[attribute]) for seq in dataset])


def one_hot_encode(labels):
    """utils.py:320-326 (an index encoding, despite the name): position of the style letter in 'CRTW'."""
    dance_types = "CRTW"
    return np.asarray([dance_types.index(l) for l in labels]).astype(int)


def get_positions(sequence, length=120):
    """utils.py:245-248: a random crop [s, s + length) drawn from numpy's global generator."""
    s = np.random.randint(0, len(sequence) - length)
    return s, s + length


def retime_sequence(frames, new_len):
    """A take of len(frames) frames re-timed to new_len frames by linear interpolation, host fp64 - the recipe in the
    comment of the reference's utils.interpolate (utils.py:257-264), which its README asks for on the waltz takes:
    out[i] = interpolate(frames, i delta), delta = (len - 1) / (new_len - 1); interpolate(x, fi) = x[i] when the
    fraction f = fi - int(fi) is below machine epsilon, else x[i] + f (x[i + 1] - x[i]). The last output is the last
    frame: where rounding leaves i delta a hair off len - 1 the reference reads x[len]; here the position is clamped."""
    x = np.asarray(frames, dtype=np.float64)
    n, new_len = len(x), int(new_len)
    if n < 1 or new_len < 1:
        raise ValueError("retime_sequence: a take of at least one frame and new_len >= 1 expected")
    if new_len == 1 or n == 1:
        return np.repeat(x[:1], new_len, axis=0)
    delta = (n - 1) / float(new_len - 1)
    pos = np.minimum(np.arange(new_len) * delta, float(n - 1))
    pos[-1] = n - 1
    i = pos.astype(np.int64)
    f = pos - i
    nxt = np.minimum(i + 1, n - 1)
    f = f.reshape((-1,) + (1,) * (x.ndim - 1))
    return np.where(f < np.finfo(np.float64).eps, x[i], x[i] + f * (x[nxt] - x[i]))


# --------------------------------------------------------------------------------------- augmentation
# One rule, stated here on the host in fp64 (augment_window); kernels.crop_augment (m2d_crop_augment) applies it inside
# the resident gather in fp32. DESIGN.md section 19.
AugmentParams = collections.namedtuple("AugmentParams", "a b mirror cos sin gain")
AugmentParams.__doc__ = """One row's augmentation: playback speed a / b (reduced, max(a, b) <= 64), mirror flag (x -> -x),
(cos, sin) of the yaw about the vertical (y) axis, audio gain factor."""
IDENTITY = AugmentParams(1, 1, False, 1.0, 0.0, 1.0)
MAX_SPEED_TERM = 64


def parse_speed(speed):
    """'a/b' (or a pair) -> (a, b): positive integers, reduced by their gcd, max(a, b) <= 64"""
    try:
        a, b = (int(v) for v in (speed.split("/") if isinstance(speed, str) else speed))
    except (TypeError, ValueError):
        raise ValueError("augment: a speed is 'a/b' with integers a and b, got %r" % (speed,))
    if a < 1 or b < 1 or max(a, b) > MAX_SPEED_TERM:
        raise ValueError("augment: speed %r: a and b must lie in [1, %d]" % (speed, MAX_SPEED_TERM))
    if math.gcd(a, b) != 1:
        raise ValueError("augment: speed %r is not reduced by its gcd (write %d/%d)" % (speed, a // math.gcd(a, b),
                                                                                     b // math.gcd(a, b)))
    return a, b


def frames_needed(T, a, b):
    """source frames a window of T output frames at speed a / b reads: ceil((T - 1) a / b) + 1"""
    return -(-(int(T) - 1) * int(a) // int(b)) + 1


def speed_taps(a, b):
    """The filter of the audio leg at speed a / b, fp64 values of the fp32 taps the device holds: audio.design_taps(b, a)
    (up = b, down = a), the one-tap identity at 1/1"""
    if a == b:
        return np.ones(1)
    from .audio import design_taps
    return design_taps(b, a)[2].astype(np.float32).astype(np.float64)


class Augment:
    """The YAML's `dataset: augment:` block -> per-row draws. Keys (all optional): mirror (probability of x -> -x, in
    [0, 1]), yaw_deg (yaw uniform in [-yaw_deg, +yaw_deg] about the vertical axis, >= 0), speeds (list of 'a/b' drawn
    uniformly), gain_db (audio gain uniform in [-gain_db, +gain_db] dB, >= 0), seed. The mirror negates x and does NOT
    exchange left and right joints: the dataset's joint names are in neither repository.
    Draws come from an own numpy Generator(seed); every row takes the same four uniforms in the same order - speed index,
    mirror, yaw, gain - whatever is switched off, so the stream does not shift with the configuration."""
    KEYS = ("mirror", "yaw_deg", "speeds", "gain_db", "seed")

    def __init__(self, cfg=None):
        cfg = dict(cfg or {})
        unknown = sorted(set(cfg) - set(self.KEYS))
        if unknown:
            raise ValueError("augment: unknown key(s) %s (known: %s)" % (", ".join(unknown), ", ".join(self.KEYS)))
        self.mirror = float(cfg.get("mirror") or 0.0)
        self.yaw_deg = float(cfg.get("yaw_deg") or 0.0)
        self.gain_db = float(cfg.get("gain_db") or 0.0)
        self.seed = int(cfg.get("seed") or 0)
        if not 0.0 <= self.mirror <= 1.0:
            raise ValueError("augment: mirror is a probability in [0, 1], got %r" % cfg.get("mirror"))
        if not (self.yaw_deg >= 0.0 and math.isfinite(self.yaw_deg)):
            raise ValueError("augment: yaw_deg must be >= 0, got %r" % cfg.get("yaw_deg"))
        if not (self.gain_db >= 0.0 and math.isfinite(self.gain_db)):
            raise ValueError("augment: gain_db must be >= 0, got %r" % cfg.get("gain_db"))
        speeds = cfg.get("speeds")
        if isinstance(speeds, str):
            speeds = [speeds]
        self.speeds = tuple(parse_speed(s) for s in (speeds or ["1/1"]))
        self.rng = np.random.Generator(np.random.PCG64(self.seed))

    def draw(self, n):
        """-> n AugmentParams, row by row; cos and sin are taken here in fp64 (the device never calls sincos)"""
        rows = []
        for _ in range(int(n)):
            u = [float(v) for v in self.rng.random(4)]
            a, b = self.speeds[min(int(u[0] * len(self.speeds)), len(self.speeds) - 1)]
            theta = math.radians((2.0 * u[2] - 1.0) * self.yaw_deg)
            gain = 10.0 ** ((2.0 * u[3] - 1.0) * self.gain_db / 20.0)
            rows.append(AugmentParams(a, b, bool(u[1] < self.mirror), math.cos(theta), math.sin(theta), gain))
        return rows


def _is_identity_pose(p):
    return not p.mirror and p.cos == 1.0 and p.sin == 0.0


def augment_window(poses_take, track_take, p0, T, S, hop, params, scaler):
    """THE rule, host fp64: the window of T frames (and S samples) that starts at frame p0 (sample p0 hop) of one take,
    under `params` -> (poses (T, J, 3), audio (S,) or None when track_take is None).
    Poses: output frame i shows source position p0 + i a / b in exact integers, j = (i a) div b, f = ((i a) mod b) / b:
    x[j] when f == 0, else x[j] + f (x[j + 1] - x[j]) (retime_sequence's recipe with an exact fraction), interpolated in
    the stored (scaled) values; then, unless the transform is the identity: un-scale per column (v - min_) / scale_,
    x -> -x under the mirror, x' = c x + s z, z' = -s x + c z (y, column 1 of a joint, is the vertical axis and the
    skeletons are centred on the body), scale again; no clamp to [0, 1]. scaler None: scale 1, shift 0.
    Audio: output n sits at source time p0 hop + n a / b: m2d_resample_poly's formula with up = b, down = a and
    speed_taps(a, b), y[n] = gain sum_m taps[n a + half - m b] X[m], X[m] = sample p0 hop + m of the take, zero outside
    the take (m may be negative); 1/1: gain X[n]."""
    a, b = int(params.a), int(params.b)
    x = np.asarray(poses_take, dtype=np.float64)
    L = len(x)
    x = x.reshape(L, -1)
    p0, T, S, hop = int(p0), int(T), int(S), int(hop)
    if p0 < 0 or p0 + frames_needed(T, a, b) > L:
        raise ValueError("augment_window: %d frames from %d at speed %d/%d do not fit a take of %d frames"
                         % (T, p0, a, b, L))
    ia = np.arange(T, dtype=np.int64) * a
    j, r = p0 + ia // b, ia % b
    f = (r / float(b))[:, None]
    nxt = np.minimum(j + 1, L - 1)
    v = np.where(f == 0.0, x[j], x[j] + f * (x[nxt] - x[j]))
    if not _is_identity_pose(params):
        scale = 1.0 if scaler is None else np.asarray(scaler.scale_, dtype=np.float64)
        shift = 0.0 if scaler is None else np.asarray(scaler.min_, dtype=np.float64)
        u = ((v - shift) / scale).reshape(T, -1, 3)
        ux = -u[..., 0] if params.mirror else u[..., 0]
        uz = u[..., 2]
        c, s = float(params.cos), float(params.sin)
        u = np.stack((c * ux + s * uz, u[..., 1], -s * ux + c * uz), axis=-1)
        v = u.reshape(T, -1) * scale + shift
    poses = v.reshape(T, -1, 3)
    if track_take is None:
        return poses, None
    X = np.asarray(track_take, dtype=np.float64)
    a0, g = p0 * hop, float(params.gain)

    def sample(idx):
        inside = (idx >= 0) & (idx < len(X))
        return np.where(inside, X[np.clip(idx, 0, max(len(X) - 1, 0))] if len(X) else 0.0, 0.0)

    n = np.arange(S, dtype=np.int64)
    if a == b:
        return poses, g * sample(a0 + n)
    taps = speed_taps(a, b)
    t = n * a + (len(taps) - 1) // 2
    q, phi = t // b, t % b
    jj = np.arange(-(-len(taps) // b), dtype=np.int64)[None, :]
    k = phi[:, None] + jj * b
    h = np.where(k < len(taps), taps[np.minimum(k, len(taps) - 1)], 0.0)
    return poses, g * (h * sample(a0 + q[:, None] - jj)).sum(axis=1)


_TAP_BANKS = {}


def _tap_bank(device, speeds):
    """The taps of every speed but 1/1 end to end in one fp32 device buffer -> (buffer, {(a, b): (offset, ntaps)})"""
    key = (str(device), tuple(sorted(set(s for s in speeds if s[0] != s[1]))))
    bank = _TAP_BANKS.get(key)
    if bank is None:
        parts, where, off = [np.zeros(1)], {}, 1    # (never empty: the kernel's audio form wants a tap buffer)
        for a, b in key[1]:
            t = speed_taps(a, b)
            where[(a, b)] = (off, len(t))
            parts.append(t)
            off += len(t)
        bank = _TAP_BANKS[key] = (torch.as_tensor(np.concatenate(parts), dtype=torch.float32).to(device), where)
    return bank


# --------------------------------------------------------------------------------------- datasets
# Storage is columnar: every take of a dataset lives in ONE array, takes back to back, with an offsets table - poses
# (sum of frames, 23, 3) and audio (sum of samples,). `sequences` / `musics` hand out per-take views of those arrays
# (the attribute contract of utils.py:48-125), a crop is an index range into them, and a whole batch of crops is one
# gather - on the host, or on the device once `to_device()` has put the two arrays into HBM (a few hundred MB for the
# real dataset against 288 GB: the dataset is resident, the loader moves indices).
class _Ragged:
    """Takes of different lengths stored back to back. Indexing gives a view; assigning a take re-packs."""

    def __init__(self, takes, dtype=None):
        takes = [np.asarray(t) if dtype is None else np.asarray(t, dtype=dtype) for t in takes]
        self._pack(takes)

    def _pack(self, takes):
        self.starts = np.zeros(len(takes) + 1, dtype=np.int64)
        if takes:
            np.cumsum([len(t) for t in takes], out=self.starts[1:])
            self.flat = np.concatenate(takes, axis=0)
        else:
            self.flat = np.zeros((0,))
        self._dev = None

    def __len__(self):
        return len(self.starts) - 1

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(len(self)))]
        i = int(i)
        if i < 0:
            i += len(self)
        return self.flat[self.starts[i]:self.starts[i + 1]]

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    def __setitem__(self, i, take):
        takes = list(self)
        takes[int(i)] = np.asarray(take)
        self._pack(takes)

    def lengths(self):
        return np.diff(self.starts)

    def map_rows(self, fn):
        """flat <- fn(flat) on all takes at once (row count unchanged)."""
        out = fn(self.flat)
        assert len(out) == len(self.flat)
        self.flat, self._dev = out, None

    def keep_heads(self, counts):
        """Truncate take i to its first counts[i] rows."""
        counts = np.minimum(np.asarray(counts, dtype=np.int64), self.lengths())
        rows = np.concatenate([np.arange(s, s + c) for s, c in zip(self.starts[:-1], counts)]) if len(self) else []
        self.flat = self.flat[rows]
        self.starts = np.concatenate([[0], np.cumsum(counts)])
        self._dev = None

    def device(self, device, dtype=torch.float32):
        if self._dev is None or self._dev.device != torch.device(device):
            self._dev = torch.from_numpy(np.ascontiguousarray(self.flat)).to(device=device, dtype=dtype)
        return self._dev


def _flatten_features(a):
    return a.reshape(len(a), -1)


class StickDataset(Dataset):
    """All still poses of the dataset, (N, 23, 3); optionally MinMax-scaled to [0, 1] - phase 1's samples, and the
    scaler every phase shares. Interface of utils.py:15-45: `name` = dataset folder, or with resume=True an .npy
    file / array of poses; centering=False adds the per-frame body centre back; attributes skeletons / centers / scaler."""

    def __init__(self, name, resume=False, centering=True, normalize=None):
        if resume:
            poses = np.load(name) if isinstance(name, (str, bytes, os.PathLike)) else np.asarray(name)
        else:
            takes = load_sticks(name)
            poses = stickwise(takes, "skeletons")
            self.centers = stickwise(takes, "center")
            if not centering:
                poses = poses + self.centers[:, None, :]
        self.scaler = None
        if normalize == "minmax":
            self.scaler = MinMaxScaler().fit(_flatten_features(poses))
            poses = self.scaler.transform(_flatten_features(poses)).reshape(poses.shape)
        self.skeletons = poses

    static_items = True  # an item is a fixed row (ResidentLoader gathers a whole epoch at once)

    def __len__(self):
        return self.skeletons.shape[0]

    def __getitem__(self, idx):
        return torch.as_tensor(self.skeletons[idx], dtype=torch.float32)

    def sample_batch(self, indices, device=None):
        """default_collate([self[i] for i in indices]) as ONE row gather - from the HBM-resident copy with `device`."""
        where = device if device is not None else "cpu"
        if getattr(self, "_dev", None) is None or self._dev.device != torch.device(where):
            self._dev = torch.as_tensor(self.skeletons, dtype=torch.float32).to(where)
        return self._dev[torch.as_tensor([int(i) for i in indices], device=where)]

    def statistics(self):
        return self.skeletons.mean(axis=0), self.skeletons.std(axis=0)

    def export(self, path):
        np.save(path, self.skeletons)


class SequenceDataset(Dataset):
    """Pose takes (+ their audio tracks); an item is a random window of `seq_length` seconds (utils.py:48-125).
    `name`: the dataset folder, or with resume=True a dict {'sequences', 'labels', 'dirs'[, 'musics']}.
    `crop_rng` (extension): a numpy RandomState / Generator the window starts are drawn from; default = numpy's global
    generator, which is what the reference draws from (utils.py:245-248), so seeded runs crop identically.
    `sync` (extension): trim the takes that have an accepted sync.json (load_all; the YAML key dataset.sync, off by
    default).
    `augment` (extension): None (off: every path is what it is without the argument), an `Augment` or the dict it is made
    from (the YAML key dataset.augment). An item is then a window under freshly drawn AugmentParams: `sample_batch` on a
    HIP device draws on the host, uploads one small table and makes ONE m2d_crop_augment launch; on the host
    (`device=None`, `__getitem__`) the same rule runs in fp64 (augment_window). A window at speed a / b needs
    frames_needed(T, a, b) frames and its start is drawn, after the row's parameters, from [0, L - need)."""

    def __init__(self, name, config, resume=False, scaler=None, dance_types=("W", "C", "R", "T"), withaudio=False,
                 crop_rng=None, sync=False, augment=None):
        self.aud_rate, self.vid_rate = config["audio_rate"], config["video_rate"]
        self.seq_length, self.feat_size = config["seq_length"], config["feat_size"]
        self.stick_length = int(self.seq_length * self.vid_rate)
        self.audio_length = int(self.seq_length * self.aud_rate)
        self.ratio = int(self.aud_rate / self.vid_rate)
        self.withaudio = withaudio
        self.crop_rng = crop_rng
        self.scaler = scaler
        self.augment = Augment(augment) if isinstance(augment, dict) else augment
        self.pose_scaler = scaler   # the scaler the stored poses are in (a subset keeps it; its `scaler` stays None)
        if resume:
            poses, self.labels, self.dirs = name["sequences"], name["labels"], name["dirs"]
            tracks = name["musics"] if withaudio else None
        else:
            takes, tracks, letters, self.dirs = load_all(name, list(dance_types), sync=sync)
            self.labels = one_hot_encode(letters)
            poses = [t["skeletons"] for t in takes]
        self._poses = _Ragged(poses)
        self._tracks = None if tracks is None else _Ragged(tracks)
        if scaler is not None:  # one transform over every frame of every take
            self._poses.map_rows(lambda f: scaler.transform(_flatten_features(f)).reshape(f.shape))

    # the reference's attribute surface: per-take arrays (views of the columnar store)
    @property
    def sequences(self):
        return self._poses

    @property
    def musics(self):
        if self._tracks is None:
            raise AttributeError("musics")
        return self._tracks

    @musics.setter
    def musics(self, tracks):
        self._tracks = tracks if isinstance(tracks, _Ragged) else _Ragged(tracks)

    def __len__(self):
        return len(self._poses)

    def _draw_start(self, idx):
        span = int(self._poses.starts[idx + 1] - self._poses.starts[idx]) - self.stick_length
        rng = self.crop_rng if self.crop_rng is not None else np.random
        draw = getattr(rng, "integers", None) or rng.randint
        return int(draw(0, span))

    # ---- augmented windows (self.augment set)
    def _draw_start_for(self, idx, p):
        """the start of a window at speed p.a / p.b, from [0, L - need) (at 1/1 the draw of _draw_start)"""
        L = int(self._poses.starts[idx + 1] - self._poses.starts[idx])
        need = frames_needed(self.stick_length, p.a, p.b)
        if L <= need:
            raise ValueError("take %s has %d frames: a window of %d frames at speed %d/%d needs more than %d"
                             % (self.dirs[idx], L, self.stick_length, p.a, p.b, need))
        rng = self.crop_rng if self.crop_rng is not None else np.random
        draw = getattr(rng, "integers", None) or rng.randint
        return int(draw(0, L - need))

    def _unit_coeffs(self, device):
        """scale 1 and shift 0 on `device`: the kernel's scaler when the poses are stored unscaled"""
        c = getattr(self, "_unit", None)
        if c is None or c[0].device != torch.device(device) or c[0].numel() != self._pose_columns():
            n = self._pose_columns()
            c = self._unit = (torch.ones(n, dtype=torch.float32, device=device),
                              torch.zeros(n, dtype=torch.float32, device=device))
        return c

    def _pose_columns(self):
        return int(np.prod(self._poses.flat.shape[1:]))

    def gather_augmented(self, indices, firsts, params, device=None):
        """The windows of takes `indices` that start at frames `firsts`, under `params` (one AugmentParams a row) ->
        (poses (B, T, J, 3) fp32, audio (B, S) fp32 or None without audio). On a HIP `device`: the per-row table of
        include/m2d.h and one m2d_crop_augment launch over the resident store; else augment_window row by row."""
        T, S, hop = self.stick_length, self.audio_length if self.withaudio else 0, self.ratio
        where = torch.device(device if device is not None else "cpu")
        if where.type != "cuda":
            rows = [augment_window(self._poses[i], self._tracks[i] if self.withaudio else None, f, T, S, hop, p,
                                   self.pose_scaler) for i, f, p in zip(indices, firsts, params)]
            poses = torch.as_tensor(np.stack([r[0] for r in rows]), dtype=torch.float32)
            audio = torch.as_tensor(np.stack([r[1] for r in rows]), dtype=torch.float32) if self.withaudio else None
            return poses, audio
        table = np.zeros(len(indices), dtype=kernels.AUGMENT_ROW)
        idx = np.asarray(indices, dtype=np.int64)
        table["pose_first"] = self._poses.starts[idx]
        table["pose_last"] = self._poses.starts[idx + 1] - 1
        table["pose_start"] = table["pose_first"] + np.asarray(firsts, dtype=np.int64)
        bank, slots = (None, {})
        if self.withaudio:
            table["audio_first"] = self._tracks.starts[idx]
            table["audio_last"] = self._tracks.starts[idx + 1] - 1
            table["audio_start"] = table["audio_first"] + np.asarray(firsts, dtype=np.int64) * hop
            speeds = self.augment.speeds if self.augment is not None else ()
            if any((p.a, p.b) not in speeds for p in params):
                speeds = tuple(speeds) + tuple((p.a, p.b) for p in params)
            bank, slots = _tap_bank(where, speeds)
        for r, p in enumerate(params):
            table[r]["a"], table[r]["b"], table[r]["mirror"] = p.a, p.b, bool(p.mirror)
            table[r]["tap_offset"], table[r]["ntaps"] = slots.get((p.a, p.b), (0, 1))
            table[r]["cos_yaw"], table[r]["sin_yaw"], table[r]["gain"] = p.cos, p.sin, p.gain
        scale, shift = self.pose_scaler._coeffs(where, False) if self.pose_scaler is not None else self._unit_coeffs(where)
        store = self._poses.device(where)
        poses, audio = kernels.crop_augment(store.view(store.shape[0], -1),
                                            self._tracks.device(where) if self.withaudio else None, table, scale,
                                            shift, bank, T, S)
        return poses.view(len(indices), T, *store.shape[1:]), audio

    def _sample_batch_augmented(self, indices, device):
        params = self.augment.draw(len(indices))
        firsts = [self._draw_start_for(i, p) for i, p in zip(indices, params)]
        poses, audio = self.gather_augmented(indices, firsts, params, device)
        where = device if device is not None else "cpu"
        labels = torch.as_tensor(np.asarray([self.labels[i] for i in indices]), device=where)
        dirs = tuple(self.dirs[i] for i in indices)
        lengths = [self.stick_length] * len(indices)
        if not self.withaudio:
            return poses, lengths, labels, dirs
        return poses, lengths, audio, labels, dirs

    def __getitem__(self, idx):
        idx = int(idx)
        if self.augment is not None:
            p = self.augment.draw(1)[0]
            first = self._draw_start_for(idx, p)
            poses, audio = augment_window(self._poses[idx], self._tracks[idx] if self.withaudio else None, first,
                                          self.stick_length, self.audio_length, self.ratio, p, self.pose_scaler)
            item = [torch.from_numpy(poses)] + ([torch.from_numpy(audio).float()] if self.withaudio else [])
            return (*item, torch.as_tensor(np.asarray(self.labels[idx])), self.dirs[idx])
        first = self._draw_start(idx)
        item = [torch.from_numpy(self._poses[idx][first:first + self.stick_length])]
        if self.withaudio:
            a0 = first * self.ratio
            item.append(torch.from_numpy(self._tracks[idx][a0:a0 + self.audio_length]).float())
        return (*item, torch.as_tensor(np.asarray(self.labels[idx])), self.dirs[idx])

    def sample_batch(self, indices, device=None):
        """A whole batch of windows in one gather - from the HBM-resident store when `device` is given. Same draws, in
        the order of `indices`, and same result as collate_fn([self[i] for i in indices], device=device) (all windows
        have equal length, so the collate step's sort is the identity): (poses, lengths, [audio,] labels, dirs)."""
        indices = [int(i) for i in indices]
        if self.augment is not None:
            return self._sample_batch_augmented(indices, device)
        firsts = np.asarray([self._draw_start(i) for i in indices], dtype=np.int64)
        rows = self._poses.starts[indices] + firsts
        where = device if device is not None else "cpu"
        t = torch.arange(self.stick_length, device=where)
        poses = self._poses.device(where)[torch.as_tensor(rows, device=where)[:, None] + t]
        labels = torch.as_tensor(np.asarray([self.labels[i] for i in indices]), device=where)
        dirs = tuple(self.dirs[i] for i in indices)
        lengths = [self.stick_length] * len(indices)
        if not self.withaudio:
            return poses, lengths, labels, dirs
        cols = self._tracks.starts[indices] + firsts * self.ratio
        s = torch.arange(self.audio_length, device=where)
        audio = self._tracks.device(where)[torch.as_tensor(cols, device=where)[:, None] + s]
        return poses, lengths, audio, labels, dirs

    def resample_audio(self, new_rate):
        from scipy.signal import resample
        factor = new_rate / self.aud_rate
        self._tracks = _Ragged([resample(t, int(len(t) * factor)) for t in self._tracks])
        self.aud_rate, self.ratio = new_rate, int(new_rate / self.vid_rate)
        self.audio_length = int(self.seq_length * new_rate)

    def truncate(self):
        """Poses and audio of every take cut to the whole seconds both have (utils.py:109-116)."""
        seconds = np.minimum((self._tracks.lengths() / self.aud_rate).astype(np.int64),
                             (self._poses.lengths() / self.vid_rate).astype(np.int64))
        self._tracks.keep_heads((seconds * self.aud_rate).astype(np.int64))
        self._poses.keep_heads((seconds * self.vid_rate).astype(np.int64))

    def subset(self, indices, withaudio=None, augment=None):
        """A dataset over the takes `indices` (same rates / crop source). `augment`: the subset's augmentation - the
        default DROPS it (a validation or classifier subset is never augmented; make_loaders hands the dataset's own to
        the train subset only)."""
        withaudio = self.withaudio if withaudio is None else withaudio
        state = {"sequences": [self._poses[i] for i in indices], "labels": [self.labels[i] for i in indices],
                 "dirs": [self.dirs[i] for i in indices]}
        if withaudio:
            state["musics"] = [self._tracks[i] for i in indices]
        cfg = {"audio_rate": self.aud_rate, "video_rate": self.vid_rate, "seq_length": self.seq_length,
               "feat_size": self.feat_size}
        sub = SequenceDataset(state, cfg, resume=True, withaudio=withaudio, crop_rng=self.crop_rng, augment=augment)
        sub.pose_scaler = self.pose_scaler
        return sub

    def export(self, pathfile):
        with open(pathfile, "wb") as f:
            pickle.dump({"sequences": list(self._poses), "labels": self.labels, "dirs": self.dirs}, f)


def collate_fn(batch, withaudio=True, device=None):
    """Ragged samples -> one zero-padded batch, longest sample first (what pack_padded_sequence wants; utils.py:128-144):
    (poses (B, Tmax, 23, 3) fp32, lengths, [audio (B, S),] labels (B,), dirs). The padding is ONE masked gather over
    the concatenated frames instead of a copy per sample; with `device` the frames are moved first and gather, mask
    and the other tensors are made there."""
    order = sorted(range(len(batch)), key=lambda i: -len(batch[i][0]))  # stable: ties keep their order, like list.sort
    cols = list(zip(*(batch[i] for i in order)))
    frames, dirs, labels = cols[0], cols[-1], torch.stack(cols[-2])
    lengths = [len(f) for f in frames]
    where = device if device is not None else frames[0].device
    flat = torch.cat([f.reshape(len(f), -1) for f in frames]).to(device=where, dtype=torch.float32, non_blocking=True)
    n = torch.as_tensor(lengths, device=where)
    t = torch.arange(max(lengths), device=where)
    inside = t[None, :] < n[:, None]                                      # (B, Tmax)
    src = (torch.cumsum(n, 0) - n)[:, None] + torch.where(inside, t[None, :], torch.zeros_like(t)[None, :])
    padded = (flat[src] * inside[..., None]).reshape(len(frames), len(t), *frames[0].shape[1:])
    labels = labels.to(where, non_blocking=True)
    if not withaudio:
        return padded, lengths, labels, dirs
    return padded, lengths, torch.stack(cols[1]).to(where, non_blocking=True), labels, dirs


class ResidentLoader:
    """`DataLoader(dataset, batch_size, sampler=sampler, drop_last=..., collate_fn=collate_fn)` for a dataset that lives
    in HBM: the train scripts' loaders (phase1/train_wgan-gp.py:71-72, phase2/train.py:115-116, phase3/train.py:150-162)
    fetch 64 items and collate them on the host, 5-33 ms per batch against 0.8-12 ms of GPU work per loop body; here the
    whole dataset (the 61 takes of the reference's data are < 1 GB of fp32) is uploaded once and a batch is the sampler's
    indices + the window draws on the host and ONE gather on the device (`dataset.sample_batch(indices, device)`).
    Draw for draw the DataLoader's stream: its iterator's base-seed draw from torch's global generator, the sampler's
    draws, the datasets' crop draws in item order - a seeded run sees the same batches either way
    (tests/test_data_pipeline.py). `sampler` is any torch sampler over item indices."""

    def __init__(self, dataset, batch_size, sampler, device, drop_last=False):
        self.dataset, self.sampler, self.device = dataset, sampler, device
        self.batch_size, self.drop_last = int(batch_size), bool(drop_last)

    def __len__(self):
        n = len(self.sampler)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def __iter__(self):
        torch.empty((), dtype=torch.int64).random_()  # (what a DataLoader iterator draws for its workers' base seed)
        if getattr(self.dataset, "static_items", False):
            # items without per-draw randomness (still poses): the whole epoch in ONE gather, batches are views of it
            order = list(self.sampler)
            rows = self.dataset.sample_batch(order, self.device) if order else None
            stop = len(order) - (len(order) % self.batch_size if self.drop_last else 0)
            for i in range(0, stop, self.batch_size):
                yield rows[i:i + self.batch_size]
            return
        chunk = []
        for i in self.sampler:
            chunk.append(i)
            if len(chunk) == self.batch_size:
                yield self.dataset.sample_batch(chunk, self.device)
                chunk = []
        if chunk and not self.drop_last:
            yield self.dataset.sample_batch(chunk, self.device)


# --------------------------------------------------------------------------------------- split + samplers
def split_indices(dataset_size, validation_split=.2, test_split=.5, random_seed=14):
    """The seeded hold-out of phase3/train.py:112-124 -> (train, val, test) index lists: a permutation of range(n)
    under numpy seed 14; its first floor(.2 n) entries are held out, the first floor(half) of those for test. Seeds
    numpy's GLOBAL generator like the reference does (the crops drawn afterwards depend on that state)."""
    np.random.seed(random_seed)
    perm = np.random.permutation(dataset_size).tolist()
    held = int(validation_split * dataset_size)
    test = int(test_split * held)
    return perm[held:], perm[test:held], perm[:test]


def class_balanced_weights(labels, indices):
    """phase3/train.py:132-143: per-sample weight = 1 / (number of samples of its style among `indices`)."""
    labels = np.asarray(labels)
    # (the reference indexes 1/counts with the label itself, which needs every style 0..k-1 present in the subset;
    # indexing through the inverse map gives the same weights then and still works when a style is missing)
    _, inverse, counts = np.unique(labels[indices], return_inverse=True, return_counts=True)
    return (1. / counts)[inverse]


def make_loaders(dataset, batch_size, withaudio=True, logdir=None, device=None):
    """Train / validation loaders over the seeded split (phase3/train.py:112-162): trainvaltest_samples.json in
    `logdir`, each subset drawn through a class-balanced WeightedRandomSampler, validation served as ONE batch.
    A dataset too small to hold anything out (< 5 takes) gets no validation loader (None). `device`: the loaders keep
    their subsets in that device's memory and gather batches there (ResidentLoader; same batches as the DataLoader)."""
    from torch.utils.data import DataLoader, WeightedRandomSampler
    parts = dict(zip(("train", "val", "test"), split_indices(len(dataset))))
    if logdir is not None:
        with open(os.path.join(logdir, "trainvaltest_samples.json"), "w") as f:
            json.dump({k + "_samples": [dataset.dirs[i] for i in v] for k, v in parts.items()}, f)

    def loader(idx, per_batch, augment=None):
        if not idx:
            return None
        weights = class_balanced_weights(dataset.labels, idx)
        sampler = WeightedRandomSampler(weights, len(weights))
        if device is not None:
            return ResidentLoader(dataset.subset(idx, withaudio, augment=augment), per_batch, sampler, device)
        return DataLoader(dataset.subset(idx, withaudio, augment=augment), batch_size=per_batch, sampler=sampler,
                          collate_fn=lambda b: collate_fn(b, withaudio=withaudio))

    # (only the train subset is augmented)
    return (loader(parts["train"], batch_size, getattr(dataset, "augment", None)),
            loader(parts["val"], len(parts["val"])), tuple(parts.values()))


# --------------------------------------------------------------------------------------- synthetic dataset folder
def planted_take(frames, samples, hop, lag, stretch=1.0, seed=0):
    """A take with a known audio-motion offset -> (audio (samples,) fp64, poses (round(frames stretch), 23, 3) fp64):
    quiet noise with a decaying burst at irregular click frames c (6 to 14 frames apart, at sample c hop + 100), and a
    body that all but stops at times c + lag (in audio frames), recorded `stretch` times slower: pose frame i shows
    time i / stretch. The profile of metrics.sync_curves peaks at lag_frames = lag, factor = 1 / stretch."""
    rng = np.random.default_rng(seed)
    x = 0.05 * rng.standard_normal(samples)
    clicks, c = [], 3
    while c < frames - 2:
        clicks.append(c)
        c += int(rng.integers(6, 15))
    for c in clicks:
        p = c * hop + 100
        n = min(3000, samples - p)
        if n > 0:
            x[p:p + n] += 0.8 * np.exp(-np.arange(n) / 400.0) * rng.standard_normal(n)
    n = int(round(frames * stretch))
    t = np.arange(n) / float(stretch)
    near = np.exp(-(t[:, None] - np.asarray(clicks, dtype=np.float64)[None, :] - lag) ** 2 / (2.0 * 1.5 ** 2)).sum(axis=1)
    amp = 0.6 - 0.4 * np.minimum(1.0, near)
    return x, np.cumsum(amp[:, None, None] / stretch * (1.0 + 0.2 * rng.standard_normal((n, 23, 3))), axis=0)


def write_synthetic_dataset(folder, n_takes=8, seconds=8, audio_rate=16000, video_rate=25, seed=0,
                            styles="CRTW", planted=None):
    """A folder in the on-disk format the loaders above read (DANCE_<style>_<n>/{skeletons.json | new_skeletons.json,
    config.json, resampled_audio_extract.wav}) filled with random poses / audio: lets the train scripts' dataset
    path run end to end without the real (absent) Music-to-Dance-Motion-Synthesis data. planted: None, or a list of
    (lag, stretch) - take n is then planted_take(..., *planted[n % len(planted)]): clicks and a dance that follows them
    lag frames late (for prepare_data --sync and --waltz-factor auto)."""
    from scipy.io import wavfile
    rng = np.random.RandomState(seed)
    os.makedirs(folder, exist_ok=True)
    for n in range(n_takes):
        style = styles[n % len(styles)]
        d = os.path.join(folder, "DANCE_%s_%d" % (style, n + 1))
        os.makedirs(d, exist_ok=True)
        frames = seconds * video_rate + int(rng.randint(0, video_rate))
        walk = np.cumsum(rng.randn(frames, 23, 3) * 0.02, axis=0) + rng.randn(1, 23, 3)
        center = np.cumsum(rng.randn(frames, 3) * 0.01, axis=0)
        samples = None
        if planted is not None:
            samples = seconds * audio_rate + int(rng.randint(0, audio_rate))
            lag, stretch = planted[n % len(planted)]
            track, walk = planted_take(frames, samples, int(audio_rate / video_rate), lag, stretch, seed + n)
            frames = len(walk)
            center = np.zeros((frames, 3))
        with open(d + _skeleton_file("DANCE_%s" % style), "w") as f:
            json.dump({"skeletons": walk.tolist(), "center": center.tolist()}, f)
        with open(d + "/config.json", "w") as f:
            json.dump({"start_position": 0, "end_position": frames}, f)
        if samples is None:
            samples = seconds * audio_rate + int(rng.randint(0, audio_rate))
            pcm = np.clip(rng.randn(samples) * 3000.0, -32767, 32767).astype(np.int16)
        else:
            pcm = np.clip(np.rint(track * 8192.0), -32767, 32767).astype(np.int16)
        wavfile.write(d + "/resampled_audio_extract.wav", audio_rate, pcm)
    return folder
