#!/usr/bin/env python
"""Turns a directory of wavs at any rate and channel count into mono wavs at the model's rate, peak-normalised, on the gfx950
kernels (``Resampler`` / ``prepare_waveforms``, msmctts_amd/hip/resample.py) -- step 1 of every recipe of the reference
(examples/csmsc/scripts/audio/audio_normalization.sh: ``sox in.wav -c 1 -r $sample_rate --norm=-7 out.wav``).

    python tools/prepare_wavs.py wav_dir -o out_dir --rate 24000 [--norm -7 | --no-norm] [--preset kaiser_best | kaiser_fast]
                                 [--jobs 16] [--float]

Every ``wav_dir/<id>.wav`` is read with all its channels through ``datasets/readers.read_wav_channels`` (16-bit PCM is uploaded
as int16).  The files are grouped by source rate and channel layout, one ``Resampler`` per rate, sorted by length, ``--jobs B`` of
them per launch; an utterance's samples do not depend on its batch.  A file already at ``--rate`` is only mixed down and
normalised.  Writes ``out_dir/<id>.wav``: 16-bit PCM through the standard library's ``wave``, round-half-even(y 32768) clipped to
[-32768, 32767], no dither; with ``--float`` IEEE-float wavs through ``scipy.io.wavfile``.  The filter is the Kaiser-windowed
sinc of csrc/resample.hip, not sox's ``rate``; files too long for one launch are not streamed.  Prints the files and seconds of
audio per second of wall time, reading and writing included.
"""
import argparse
import os
import sys
import time
import wave

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'msmc-tts_amd')]
import msmctts_amd  # noqa: E402,F401
import numpy as np  # noqa: E402


def list_wavs(wav_dir):
    """[(id, path)] of the .wav files of a directory, sorted by name"""
    names = sorted(n for n in os.listdir(wav_dir) if n.lower().endswith('.wav'))
    return [(n[:-4], os.path.join(wav_dir, n)) for n in names]


def to_pcm16(y):
    """float [-1, 1) -> int16: round-half-even(y 32768), clipped; no dither"""
    return np.clip(np.rint(np.asarray(y, dtype=np.float64) * 32768.0), -32768, 32767).astype('<i2')


def write_wav(path, y, rate, as_float=False):
    if as_float:
        from scipy.io import wavfile
        wavfile.write(path, rate, np.ascontiguousarray(y, dtype=np.float32))
        return
    with wave.open(path, 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(to_pcm16(y).tobytes())


def prepare_dir(wav_dir, output_dir, rate, norm_db=-7.0, preset='kaiser_best', jobs=16, as_float=False, device='cuda', out=sys.stdout):
    """-> (files, seconds of audio read)"""
    from msmctts_amd.datasets import readers
    from msmctts_amd.hip.resample import Resampler
    start = time.time()
    groups = {}
    for uid, path in list_wavs(wav_dir):
        wav, src_rate = readers.read_wav_channels(path)
        groups.setdefault((src_rate, wav.shape[1], wav.dtype.str), []).append((uid, wav))
    if not groups:
        raise ValueError('%s holds no .wav file' % wav_dir)
    os.makedirs(output_dir, exist_ok=True)
    resamplers = {}
    files, seconds = 0, 0.0
    for (src_rate, _, _), items in sorted(groups.items()):
        if src_rate not in resamplers:
            resamplers[src_rate] = Resampler(src_rate, rate, preset=preset, device=device)
        rs = resamplers[src_rate]
        items.sort(key=lambda it: (len(it[1]), it[0]))
        for first in range(0, len(items), jobs):
            batch = items[first:first + jobs]
            y, length = rs.resample([w for _, w in batch], norm_db=norm_db)
            y, length = y.cpu().numpy(), length.cpu().tolist()
            for b, (uid, w) in enumerate(batch):
                write_wav(os.path.join(output_dir, uid + '.wav'), y[b, :int(length[b])], rate, as_float)
                files, seconds = files + 1, seconds + len(w) / float(src_rate)
    took = max(time.time() - start, 1e-9)
    print('%d files, %.1f s of audio in %.3f s: %.1f files/s, %.1f audio-seconds/s' % (files, seconds, took, files / took, seconds / took),
          file=out)
    return files, seconds


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('wav_dir')
    ap.add_argument('-o', '--output-dir', required=True)
    ap.add_argument('--rate', type=int, required=True, help='the sample rate to write, e.g. 24000')
    ap.add_argument('--norm', type=float, default=-7.0, help='peak level in dBFS (default -7, as the reference)')
    ap.add_argument('--no-norm', action='store_true', help='leave the level as it is')
    ap.add_argument('--preset', default='kaiser_best', choices=('kaiser_best', 'kaiser_fast'))
    ap.add_argument('-j', '--jobs', type=int, default=16, help='utterances per launch')
    ap.add_argument('--float', dest='as_float', action='store_true', help='write IEEE-float wavs in place of 16-bit PCM')
    ap.add_argument('--device', default='cuda', help='default: the current GPU')
    args = ap.parse_args(argv)
    if args.jobs < 1:
        ap.error('--jobs must be positive')
    return prepare_dir(args.wav_dir, args.output_dir, args.rate, None if args.no_norm else args.norm, args.preset, args.jobs,
                       args.as_float, args.device)


if __name__ == '__main__':
    main()
