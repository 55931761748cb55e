"""Music-dance beat alignment on the device (include/m2d.h "beat alignment").

Jerkiness and style agreement (phase3.evaluate) never look at the music. This module asks whether the kinematic beats
of a dance - local minima of the body's speed - fall on musical onsets, as the beat-alignment scores of AIST++ and
"Dancing to Music" do:

    audio -> STFT band energies (m2d_stft_bands: the DFT on fp32 MFMA, the mel projection fused)
          -> onset strength (m2d_onset_flux: log-compressed, rectified spectral flux)
    poses -> mean joint speed (m2d_motion_speed)
    both  -> smoothing, events, nearest-event distances, beat_align and beat_cover (m2d_beat_align)

Pose frame t belongs to samples [t hop, (t + 1) hop); STFT frame t is centred on the middle of that interval. Device
tensors in, device tensors out, no host synchronisation inside. The window, the mel bands, the smoothing widths and
gamma are conventions of this project (the reference has no such metric); all are parameters.

Distribution scores (include/m2d.h "distribution scores") ask whether a SET of generated dances
has the distribution of the real ones, as the FID_k / Div_k of AIST++ and the FID, diversity and multimodality of
"Dancing to Music" do:

    poses    -> kinetic features per joint (m2d_kinetic_features)
    features -> fp64 mean and covariance (m2d_feature_moments)
    moments  -> Frechet distance (m2d_frechet: two Jacobi eigen-solves, m2d_sym_eig's kernel, and two products)
    features -> mean pairwise distance (m2d_pairwise_mean_dist): diversity (one group), multimodality (a group per
                piece of music)

k-nearest-neighbour scores (include/m2d.h "nearest-neighbour queries") separate what one Frechet
number mixes - fidelity from variety - and ask whether a generator has memorised its training rows: improved
precision and recall (Kynkaanniemi et al. 2019), density and coverage (Naeem et al. 2020) and nearest-training-row
distances:

    rows        -> k-th nearest-neighbour radii inside a set (m2d_knn_radii)
    rows, radii -> per query: in how many balls it lies, and its nearest row of the other set (m2d_ball_query)
    both        -> prdc(real, fake, k)

Audio-motion synchronisation (include/m2d.h "audio-motion synchronisation") asks where a take's
dance sits on its music - the reference's takes are not synchronised, and its waltz takes run at another speed:

    audio, poses -> the smoothed onset curve and the negated smoothed speed curve (sync_curves: m2d_gauss_smooth)
    curves       -> their correlation over time-scale factors and integer lags (sync_profile: m2d_sync_scan)
    profile      -> factor, lag, peak, second peak (sync_estimate, host fp64)
"""
import numpy as np
import torch

from . import _lib, kernels
from .audio import _rows

N_JOINTS = 23
_BASIS = {}   # (n_fft, device) -> (fp32 table on the device, its packed image)
_BANDS = {}   # (n_bands, n_fft, rate, device) -> fp32 mel bands on the device


def mel_bands(n_bands=40, n_fft=1024, rate=16000):
    """float64 (n_bands, n_fft / 2 + 1): HTK-mel triangles of peak 1; n_bands + 2 points equally spaced in
    mel(f) = 2595 log10(1 + f / 700) from mel(0) to mel(rate / 2) are the corners f_0 .. f_{n_bands + 1};
    bands[b, k] = max(0, min((F_k - f_b) / (f_{b+1} - f_b), (f_{b+2} - F_k) / (f_{b+2} - f_{b+1}))), F_k = k rate / n_fft"""
    n_bands, n_fft = int(n_bands), int(n_fft)
    mel_hi = 2595.0 * np.log10(1.0 + (rate / 2.0) / 700.0)
    f = 700.0 * (10.0 ** (np.linspace(0.0, mel_hi, n_bands + 2) / 2595.0) - 1.0)
    F = np.arange(n_fft // 2 + 1, dtype=np.float64) * rate / n_fft
    up = (F[None, :] - f[:-2, None]) / (f[1:-1] - f[:-2])[:, None]
    down = (f[2:, None] - F[None, :]) / (f[2:] - f[1:-1])[:, None]
    return np.maximum(0.0, np.minimum(up, down))


def stft_table(n_fft):
    """The host half of stft_basis: float32 (2, n_fft / 2 + 1, n_fft), [w[n] cos(a); -w[n] sin(a)] with
    a = 2 pi ((n k) mod n_fft) / n_fft and w the periodic Hann window, evaluated in fp64 and rounded once"""
    n_fft = int(n_fft)
    if n_fft < 256 or n_fft > 2048 or n_fft & (n_fft - 1):
        raise ValueError("n_fft must be a power of two in [256, 2048], got %d" % n_fft)
    n = np.arange(n_fft, dtype=np.int64)
    k = np.arange(n_fft // 2 + 1, dtype=np.int64)
    a = 2.0 * np.pi * ((k[:, None] * n[None, :]) % n_fft).astype(np.float64) / n_fft
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * n.astype(np.float64) / n_fft)
    return np.stack((w[None, :] * np.cos(a), -w[None, :] * np.sin(a))).astype(np.float32)


def stft_basis(n_fft, device):
    """The packed basis image m2d_stft_bands reads, made once per (n_fft, device)"""
    device = torch.device(device)
    key = (int(n_fft), str(device))
    ent = _BASIS.get(key)
    if ent is None:
        if key[0] < 256 or key[0] > 2048 or key[0] & (key[0] - 1):
            raise _lib.M2dError("stft_basis: n_fft must be a power of two in [256, 2048], got %d" % key[0])
        table = torch.from_numpy(stft_table(n_fft)).to(device)
        ent = _BASIS[key] = (table, kernels.impl().stft_pack_basis(table))
    return ent[1]


def _device_bands(bands, n_fft, rate, device):
    if bands is None:
        key = (40, int(n_fft), int(rate), str(device))
        b = _BANDS.get(key)
        if b is None:
            b = _BANDS[key] = torch.as_tensor(mel_bands(40, n_fft, rate), dtype=torch.float32).to(device)
        return b
    b = torch.as_tensor(bands).detach().to(device=device, dtype=torch.float32).contiguous()
    if b.dim() != 2 or b.shape[1] != int(n_fft) // 2 + 1:
        raise ValueError("bands: (nb, n_fft / 2 + 1) expected, got %s" % (tuple(b.shape),))
    return b


def band_energies(audio, n_frames, hop, n_fft=1024, bands=None, rate=16000, frame0=0):
    """audio (N,) or (B, N) fp32 on the device -> E (B, n_frames, nb): band energies of STFT frames frame0 ..
    frame0 + n_frames - 1 (frame t is centred on t hop + hop / 2; zeros outside the track). Bit-identical however
    the frames of a track are cut into calls. bands None: mel_bands(40, n_fft, rate)."""
    x = _rows(audio)
    return kernels.impl().stft_bands(x, int(n_frames), int(hop), int(n_fft), stft_basis(n_fft, x.device),
                                     _device_bands(bands, n_fft, rate, x.device), int(frame0))


def onset_strength(audio, n_frames, hop, n_fft=1024, bands=None, rate=16000, gamma=1.0):
    """-> o (B, n_frames): o[0] = 0, o[t] = mean over bands of max(0, L[t] - L[t - 1]), L = log1p(gamma E)"""
    return kernels.impl().onset_flux(band_energies(audio, n_frames, hop, n_fft, bands, rate), gamma)


def _pose_rows(poses):
    p = torch.as_tensor(poses)
    if p.dim() >= 2 and p.shape[-1] != 3:      # (..., T, 3 J)
        if p.shape[-1] % 3:
            raise ValueError("poses: (B, T, J, 3) or (B, T, 3 J) expected, got %s" % (tuple(p.shape),))
        p = p.reshape(p.shape[:-1] + (p.shape[-1] // 3, 3))
    if p.dim() == 3:
        p = p.unsqueeze(0)
    if p.dim() != 4:
        raise ValueError("poses: (B, T, J, 3) or (B, T, 3 J) expected, got %s" % (tuple(p.shape),))
    return p.contiguous()


def motion_speed(poses):
    """poses (B, T, J, 3) or (B, T, 3 J) (one dance: (T, J, 3) or (T, 3 J)) in world units, T >= 2 -> v (B, T):
    v[t] = mean over joints of |p[t] - p[t - 1]|, v[0] = v[1]"""
    return kernels.impl().motion_speed(_pose_rows(poses))


def beat_alignment(onset, speed, sigma_onset=1.0, sigma_speed=2.0, sigma_align=2.0, return_events=False):
    """onset, speed (B, T) -> {'align', 'cover', 'n_motion', 'n_music'} (B,) device tensors; align = mean over
    kinematic beats of exp(-d^2 / (2 sigma_align^2)), d the distance (frames) to the nearest musical onset; cover the
    same over the onsets; both NaN where a row has no kinematic beat or no onset. return_events: also
    'motion_events', 'music_events' (B, T) uint8 and 'onset_smooth', 'speed_smooth' (B, T)."""
    out = kernels.impl().beat_align(onset, speed, sigma_onset, sigma_speed, sigma_align, return_events)
    scores = out[0] if return_events else out
    res = {"align": scores[:, 0], "cover": scores[:, 1], "n_motion": scores[:, 2], "n_music": scores[:, 3]}
    if return_events:
        res.update(motion_events=out[1], music_events=out[2], onset_smooth=out[3], speed_smooth=out[4])
    return res


def beat_scores(audio, poses, hop, rate=16000, n_fft=1024, bands=None, gamma=1.0, **kw):
    """audio (B, N) at `rate` Hz and the dances poses (B, T, J, 3) / (B, T, 3 J) it accompanies, `hop` samples a pose
    frame -> beat_alignment(...) of the onset strength of the T frames against the motion speed; **kw: its sigmas
    and return_events"""
    p = _pose_rows(poses)
    x = _rows(audio)
    if x.shape[0] != p.shape[0]:
        raise ValueError("beat_scores: %d audio rows for %d dances" % (x.shape[0], p.shape[0]))
    onset = onset_strength(x, p.shape[1], hop, n_fft, bands, rate, gamma)
    return beat_alignment(onset, motion_speed(p), **kw)


# --------------------------------------------------------------------------- audio-motion synchronisation of a take
def sync_curves(audio, poses, hop, rate=16000, n_fft=1024, bands=None, gamma=1.0, sigma_onset=1.0, sigma_speed=2.0):
    """The two curves whose correlation places a dance on its music, for one take or a batch of
    equal-length takes: audio (N,) / (B, N) at `rate` Hz, poses (T, J, 3) / (B, T, J, 3) / (.., T, 3 J), `hop` samples a
    pose frame -> (a (B, ceil(N / hop)), b (B, T)):
        a = g(onset_strength(audio), sigma_onset)       peaks on the musical onsets
        b = -g(motion_speed(poses), sigma_speed)        peaks where the dancer stops (motion events are speed minima)
    g is the smoothing of beat_alignment (m2d_gauss_smooth). The two lengths differ when audio and poses do."""
    p = _pose_rows(poses)
    x = _rows(audio)
    if x.shape[0] != p.shape[0]:
        raise ValueError("sync_curves: %d audio rows for %d dances" % (x.shape[0], p.shape[0]))
    hop = int(hop)
    K = kernels.impl()
    a = K.gauss_smooth(onset_strength(x, -(-x.shape[1] // hop), hop, n_fft, bands, rate, gamma), sigma_onset)
    return a, -K.gauss_smooth(motion_speed(p), sigma_speed)


def _row_lengths(n, rows, device):
    if n is None:
        return None
    t = torch.as_tensor(n).to(device=device, dtype=torch.int32).reshape(-1).contiguous()
    if t.numel() != rows:
        raise ValueError("sync_profile: %d lengths for %d rows" % (t.numel(), rows))
    return t


def sync_profile(a, b, factors=(1.0,), max_lag=250, min_overlap=64, na=None, nb=None):
    """a (B, Ta), b (B, Tb) fp32 curves on the device (one row: (Ta,), (Tb,)), na / nb optional per-row lengths ->
    (r (B, F, 2 max_lag + 1) fp64, n int32): r[., i, l + max_lag] is the Pearson correlation of a[j] with b read at
    (j + l) / factors[i] (linear interpolation), over the n pairs whose position lies in b; NaN where n < min_overlap
    or a variance is zero. l > 0: the motion lags the audio by l frames; a factor f is what retime_sequence would be
    given (new length round(Tb f)). One m2d_sync_scan launch for the whole batch."""
    a, b = _rows(a), _rows(b)
    return kernels.impl().sync_scan(a, b, factors, int(max_lag), int(min_overlap),
                                    _row_lengths(na, a.shape[0], a.device), _row_lengths(nb, a.shape[0], a.device))


SYNC_WINDOW = 3   # r_second looks outside |l - l*| <= SYNC_WINDOW


def sync_estimate(r, n, factors, max_lag):
    """The profile of sync_profile -> one dict per row: 'factor' and 'lag_frames' = the (f*, l*) of the largest non-NaN
    r (ties: the smallest |l|, then the first factor), 'r' its value, 'overlap' its n, 'r_second' the largest r of the
    same factor outside |l - l*| <= 3, 'lag' the parabolic sub-frame refinement through l* - 1, l*, l* + 1 (= l* at the
    grid's edge, next to a NaN, or on a flat top; reported only - what is applied is lag_frames). A row without any
    defined r, or a missing r_second, gives None. Host fp64 on the copied profile."""
    R = np.asarray(torch.as_tensor(r).detach().cpu().numpy(), dtype=np.float64)
    N = np.asarray(torch.as_tensor(n).detach().cpu().numpy())
    L = int(max_lag)
    factors = [float(f) for f in factors]
    if R.ndim != 3 or R.shape[1:] != (len(factors), 2 * L + 1) or N.shape != R.shape:
        raise ValueError("sync_estimate: r and n (B, %d, %d) expected, got %s and %s"
                         % (len(factors), 2 * L + 1, R.shape, N.shape))
    lags = np.arange(-L, L + 1)
    out = []
    for row, cnt in zip(R, N):
        ok = ~np.isnan(row)
        if not ok.any():
            out.append({"factor": None, "lag_frames": None, "lag": None, "r": None, "r_second": None, "overlap": 0})
            continue
        top = row[ok].max()
        cand = [(abs(int(lags[k])), i, k) for i, k in zip(*np.nonzero(ok & (row == top)))]
        _, i, k = min(cand)
        prof = row[i]
        lag = float(lags[k])
        if 0 < k < 2 * L and not np.isnan(prof[k - 1]) and not np.isnan(prof[k + 1]):
            den = prof[k - 1] - 2.0 * prof[k] + prof[k + 1]
            if den != 0.0:
                lag += 0.5 * (prof[k - 1] - prof[k + 1]) / den
        rest = prof[(np.abs(lags - lags[k]) > SYNC_WINDOW) & ~np.isnan(prof)]
        out.append({"factor": factors[i], "lag_frames": int(lags[k]), "lag": lag, "r": float(top),
                    "r_second": float(rest.max()) if rest.size else None, "overlap": int(cnt[i, k])})
    return out


# ------------------------------------------------------------------------------------------- distribution scores
def kinetic_features(poses, fps=25.0, up_axis=1):
    """poses (B, T, J, 3) or (B, T, 3 J) (one dance: (T, J, 3) or (T, 3 J)) in world units, T >= 3 -> F (B, 3 J) fp32,
    [h_0 .. h_{J-1} | v_0 .. | e_0 ..]: per joint the mean squared horizontal speed (the two axes other than
    `up_axis`), the mean squared vertical speed and the mean absolute acceleration, with v[t] = (p[t] - p[t - 1]) fps
    and a[t] = (p[t + 1] - 2 p[t] + p[t - 1]) fps^2"""
    return kernels.impl().kinetic_features(_pose_rows(poses), float(fps), int(up_axis))


def feature_moments(X):
    """X (N, D) fp32, N >= 2 -> (mean (D), cov (D, D)) fp64, cov unbiased (N - 1) and exactly symmetric"""
    return kernels.impl().feature_moments(X)


def sym_eig(A, vectors=False):
    """A (D, D) or (P, D, D) fp64 symmetric -> {'values' (.., D) ascending, 'sweeps', 'converged' (..,)} and, with
    `vectors`, 'vectors' (.., D, D): the eigenvectors as columns. A matrix with a NaN or an infinity gives NaN values
    and converged 0 after the solver's fixed number of sweeps."""
    A3 = A.unsqueeze(0) if A.dim() == 2 else A
    w, V, info = kernels.impl().sym_eig(A3.contiguous(), vectors)
    lead = A.shape[:-2]
    res = {"values": w.reshape(lead + w.shape[-1:]), "sweeps": info[:, 0].reshape(lead),
           "converged": info[:, 1].reshape(lead)}
    if vectors:
        res["vectors"] = V.reshape(A.shape)
    return res


FRECHET_FIELDS = ("fd", "mean_term", "trace_term", "sqrt_term", "sweeps", "converged")


def frechet_from_moments(m1, S1, m2, S2):
    """means (D) / (P, D) and covariances (D, D) / (P, D, D), fp64 -> {'fd', 'mean_term', 'trace_term', 'sqrt_term',
    'sweeps', 'converged'}, 0-dim (or (P,)) fp64 tensors: fd = mean_term + trace_term - 2 sqrt_term with mean_term =
    |m1 - m2|^2, trace_term = tr S1 + tr S2, sqrt_term = tr (S1 S2)^1/2. fd is NOT clipped at zero: two equal samples
    may give a tiny negative number. All pairs of a call go through one m2d_frechet launch sequence."""
    single = m1.dim() == 1
    args = [t.unsqueeze(0) if single else t for t in (m1, S1, m2, S2)]
    out = kernels.impl().frechet(*[t.contiguous() for t in args])
    return {k: (out[0, i] if single else out[:, i]) for i, k in enumerate(FRECHET_FIELDS)}


def frechet_distance(X1, X2):
    """X1 (N1, D), X2 (N2, D) fp32 feature rows -> frechet_from_moments of their moments"""
    m1, S1 = feature_moments(X1)
    m2, S2 = feature_moments(X2)
    return frechet_from_moments(m1, S1, m2, S2)


def mean_pairwise_distance(X, groups=1):
    """X (G K, D) fp32, `groups` = G groups of K consecutive rows -> (G,) fp64: the mean Euclidean distance over the
    K (K - 1) / 2 pairs of each group; NaN for K = 1. Diversity is groups = 1; multimodality is the mean over the
    groups when a group holds the dances made for one piece of music."""
    return kernels.impl().pairwise_mean_dist(X, int(groups))


def standardize(X, mean, cov):
    """(x - mean) / sqrt(diag cov) per column, fp32; a column whose variance is 0 is divided by 1"""
    var = torch.diagonal(cov)
    sd = torch.where(var > 0, var.sqrt(), torch.ones_like(var))
    return ((X.double() - mean) / sd).float().contiguous()


# ------------------------------------------------------------------------------------ k-nearest-neighbour scores
PRDC_KEYS = ("precision", "recall", "density", "coverage", "nn_ratio_median", "nn_fake_to_real_median",
             "nn_real_to_real_median")


def knn_radii(X, k=5):
    """X (N, D) fp32, N >= k + 1 -> r2 (N,) fp32: the k-th smallest SQUARED distance of row i to the rows j != i (the
    row itself is excluded by index; a duplicate of it counts). d2 = sum_d (x_d - y_d)^2, one fp32 fma chain."""
    return kernels.impl().knn_radii(X, int(k))


def ball_query(Q, P, r2=None):
    """Q (M, D), P (N, D) fp32, r2 (N,) or None -> (count (M,) int32 or None, nn_d2 (M,) fp32, nn_idx (M,) int32):
    count[j] = #{i : d2(Q_j, P_i) <= r2[i]}, nn_d2[j] = min_i d2(Q_j, P_i), nn_idx[j] the smallest i attaining it"""
    return kernels.impl().ball_query(Q, P, r2)


def _median64(x):
    s = torch.sort(x.double()).values
    n = s.numel()
    return 0.5 * (s[(n - 1) // 2] + s[n // 2])


def nearest_stats(d2):
    """d2 (n,) squared distances -> {'median', 'mean', 'min'} of their square roots, fp64 0-dim tensors on d2's device
    (the median of an even number of values is the mean of the two middle ones)"""
    d = d2.double().sqrt()
    return {"median": _median64(d), "mean": d.mean(), "min": d.min()}


def prdc(real, fake, k=5):
    """real (N, D), fake (M, D) fp32 rows, N, M >= k + 1 -> dict of fp64 0-dim device tensors (PRDC_KEYS). With
    r2_R[i] / r2_F[j] the k-th nearest-neighbour radii inside each set:
        precision = mean_j [exists i: d2(F_j, R_i) <= r2_R[i]]      density  = sum_j #{i: d2(F_j, R_i) <= r2_R[i]} / (k M)
        recall    = mean_i [exists j: d2(R_i, F_j) <= r2_F[j]]      coverage = mean_i [min_j d2(R_i, F_j) <= r2_R[i]]
        nn_fake_to_real_median = median_j sqrt(min_i d2(F_j, R_i)), nn_real_to_real_median = median_i sqrt(r2_R[i] at k = 1)
        nn_ratio_median = their quotient (NaN when the denominator is 0): well below 1, the generated rows sit closer to
        real rows than real rows sit to each other - memorisation.
    Two radii launches, the k = 1 radii and two queries (the real-to-fake query gives both the recall counts and the
    minima coverage needs); the means are integer torch reductions of the (M,) / (N,) results (the density sum in int64) and one division. No host
    read inside."""
    k = int(k)
    r2_real = knn_radii(real, k)
    r2_fake = knn_radii(fake, k)
    r2_real1 = r2_real if k == 1 else knn_radii(real, 1)
    cnt_f, nn_f, _ = ball_query(fake, real, r2_real)
    cnt_r, nn_r, _ = ball_query(real, fake, r2_fake)
    f2r = nearest_stats(nn_f)["median"]
    r2r = nearest_stats(r2_real1)["median"]
    nan = torch.full_like(r2r, float("nan"))
    # integer counts, then ONE fp64 division each, by a device tensor (a division by a Python number is carried out as a
    # multiplication by its reciprocal on the device, which rounds twice)
    def ratio(count, n):
        return count.double() / torch.full((), float(n), dtype=torch.float64, device=count.device)

    n_real, n_fake = real.shape[0], fake.shape[0]
    return {"precision": ratio((cnt_f > 0).sum(), n_fake),
            "recall": ratio((cnt_r > 0).sum(), n_real),
            "density": ratio(cnt_f.long().sum(), k * n_fake),
            "coverage": ratio((nn_r <= r2_real).sum(), n_real),
            "nn_ratio_median": torch.where(r2r > 0, f2r / torch.where(r2r > 0, r2r, torch.ones_like(r2r)), nan),
            "nn_fake_to_real_median": f2r,
            "nn_real_to_real_median": r2r}
