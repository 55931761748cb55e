"""Shared by tests/test_resample_host.py and tests/test_gpu_resample.py: the push splits of the streaming checks and a
dataset folder in the PUBLISHED layout (audio_extract.wav at the recording's own rate, the waltz take with
skeletons.json only), which prepare_data turns into what the loaders read."""
import os

import numpy as np

# take -> (style, sample rate, wav format)
RAW_TAKES = {1: ("C", 44100, "int16"), 2: ("R", 48000, "float32 stereo"), 3: ("T", 16000, "int16"),
             4: ("W", 44100, "int16")}
RAW_SECONDS = 2


def chunkings(N):
    """push sizes that sum to N: single samples first, one 10 ms block of 44.1 kHz at a time, and a ragged mix"""
    return {"ones": [1] * 50 + [N - 50],
            "441s": [441] * (N // 441) + ([N % 441] if N % 441 else []),
            "mixed": [1000, 7, 4410, 3, N - 5420]}


def raw_folder(folder):
    from scipy.io import wavfile
    from music2dance_amd.data import write_synthetic_dataset
    write_synthetic_dataset(folder, n_takes=len(RAW_TAKES), seconds=RAW_SECONDS, styles="CRTW")
    for n, (style, rate, fmt) in RAW_TAKES.items():
        d = os.path.join(folder, "DANCE_%s_%d" % (style, n))
        os.remove(os.path.join(d, "resampled_audio_extract.wav"))
        rng = np.random.RandomState(n)
        if fmt == "int16":
            data = np.clip(rng.randn(RAW_SECONDS * rate) * 3000.0, -32767, 32767).astype(np.int16)
        else:
            data = (rng.randn(RAW_SECONDS * rate, 2) * 0.1).astype(np.float32)
        wavfile.write(os.path.join(d, "audio_extract.wav"), rate, data)
    w = os.path.join(folder, "DANCE_W_4")
    os.rename(os.path.join(w, "new_skeletons.json"), os.path.join(w, "skeletons.json"))
    return folder


def listing(folder):
    """[(relative path, size, mtime in ns)] of every file below `folder`"""
    out = []
    for root, _, files in os.walk(folder):
        for f in files:
            st = os.stat(os.path.join(root, f))
            out.append((os.path.relpath(os.path.join(root, f), folder), st.st_size, st.st_mtime_ns))
    return sorted(out)
