#!/usr/bin/env python
"""Turns a directory of wavs into the ``mel/<id>.npy`` (and ``energy/<id>.npy``, ``pitch/<id>.npy``) files ``MelDataset``,
``TTSDataset`` and ``EmbDataset`` read, on the gfx950 kernels (``FeatureExtractor``, msmctts_amd/hip/features.py;
``PitchExtractor``, msmctts_amd/hip/pitch.py) -- the first step of every recipe of the reference
(examples/csmsc/scripts/audio/melspectrogram.py on a CPU process pool; the reference has no F0 tracker).

    python tools/extract_features.py wav_dir -o out_dir [--energy] [--pitch [--fmin 60] [--fmax 500] [--threshold 0.15]]
                                     [--spectrogram] [--jobs 16] [--config hparams.yaml] [--resample [--norm -7 | --norm none]]

Every ``wav_dir/<id>.wav`` is read through ``datasets/readers.py`` (first channel, integer PCM scaled to [-1, 1)).  A file whose
sample rate is not ``sample_rate`` is refused by name: resampling is not done here (the reference resamples inside
``librosa.load``) -- unless ``--resample`` is given: then every file goes through the reference's step 1 first
(``prepare_waveforms``, msmctts_amd/hip/resample.py: all channels mixed down, resampled to ``sample_rate`` where its rate differs,
peak-normalised to ``--norm`` dBFS, -7 as the reference, ``none`` to leave the level), as tools/prepare_wavs.py would have
written it but without the rounding to 16 bits.  The files are sorted by length and ``--jobs B`` of them share a launch; an utterance's features do not depend
on its batch.  Writes ``out_dir/mel/<id>.npy`` float32 [T, num_mels] and, with ``--energy``, ``out_dir/energy/<id>.npy`` float32
[T], T = 1 + samples // hop.  With ``--pitch`` the same batches also give ``out_dir/pitch/<id>.npy`` float32 [T]: YIN's
natural-log F0 on the same frame grid, 0 on unvoiced frames; ``--fmin``, ``--fmax`` and ``--threshold`` override the config's
values.  With ``--spectrogram`` the same batches also give ``out_dir/spec/<id>.npy`` float32 [T, num_freq]: the reference's
``audio.spectrogram`` (``GriffinLim.spectrogram``, msmctts_amd/hip/griffin_lim.py), what tools/invert_features.py --linear
reads.  ``--config``: a yaml file naming some of the reference's hparams (``sample_rate``, ``num_mels``,
``num_freq``, ``frame_length_ms``, ``frame_shift_ms``, ``preemphasis``, ``min_level_db``, ``ref_level_db``, ``max_abs_value``,
``symmetric_specs``; for the pitch also ``fmin``, ``fmax``, ``threshold``), at the top level or under ``hparams``; the rest keep
the defaults of hparams.py.  Prints the files, frames
and seconds of audio per second of wall time, reading and writing included.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'msmc-tts_amd')]
import msmctts_amd  # noqa: E402,F401
import numpy as np  # noqa: E402


def list_wavs(wav_dir):
    """[(id, path)] of the .wav files of a directory, sorted by name"""
    names = sorted(n for n in os.listdir(wav_dir) if n.lower().endswith('.wav'))
    return [(n[:-4], os.path.join(wav_dir, n)) for n in names]


def prepared_items(extractor, wav_dir, norm_db, jobs):
    """[(id, fp32 [L_out])]: every file through ``prepare_waveforms``, batched by source rate and channel layout"""
    from msmctts_amd.datasets import readers
    from msmctts_amd.hip.resample import Resampler, prepare_waveforms
    groups = {}
    for uid, path in list_wavs(wav_dir):
        wav, rate = readers.read_wav_channels(path)
        groups.setdefault((rate, wav.shape[1], wav.dtype.str), []).append((uid, wav))
    items, resamplers = [], {}
    for (rate, _, _), group in sorted(groups.items()):
        if rate not in resamplers:
            resamplers[rate] = Resampler(rate, extractor.sample_rate, device=extractor.device)
        group.sort(key=lambda it: (len(it[1]), it[0]))
        for first in range(0, len(group), jobs):
            batch = group[first:first + jobs]
            y, length = prepare_waveforms([w for _, w in batch], None, rate, extractor.sample_rate, norm_db=norm_db,
                                          resampler=resamplers[rate])
            y, length = y.cpu().numpy(), length.cpu().tolist()
            items += [(uid, np.ascontiguousarray(y[b, :int(length[b])])) for b, (uid, _) in enumerate(batch)]
    return items


def extract_dir(extractor, wav_dir, output_dir, energy=False, jobs=16, out=sys.stdout, pitch=None, resample=False, norm_db=-7.0,
                spectrogram=None):
    """-> (files, frames, samples).  ``pitch``: a ``PitchExtractor`` on the extractor's sample rate and hop, or None;
    ``spectrogram``: a ``GriffinLim`` of the extractor's hparams, or None.  Raises
    ``ValueError`` naming the first file at another sample rate before anything is written, unless ``resample``: then every file
    is mixed down, resampled where needed and peak-normalised to ``norm_db`` (None: not normalised) first."""
    from msmctts_amd.datasets import readers
    if pitch is not None and (pitch.sample_rate, pitch.hop) != (extractor.sample_rate, extractor.hop):
        raise ValueError('pitch at %d Hz with a hop of %d, mel at %d Hz with a hop of %d: the tracks would not line up'
                         % (pitch.sample_rate, pitch.hop, extractor.sample_rate, extractor.hop))
    items = prepared_items(extractor, wav_dir, norm_db, jobs) if resample else []
    for uid, path in ([] if resample else list_wavs(wav_dir)):
        wav, rate = readers.read_wav(path)
        if rate != extractor.sample_rate:
            raise ValueError('%s: sample rate %d, the features are defined at %d (resample it first)'
                             % (path, rate, extractor.sample_rate))
        items.append((uid, wav[:, 0]))
    if not items:
        raise ValueError('%s holds no .wav file' % wav_dir)
    os.makedirs(os.path.join(output_dir, 'mel'), exist_ok=True)
    if energy:
        os.makedirs(os.path.join(output_dir, 'energy'), exist_ok=True)
    if pitch is not None:
        os.makedirs(os.path.join(output_dir, 'pitch'), exist_ok=True)
    if spectrogram is not None:
        os.makedirs(os.path.join(output_dir, 'spec'), exist_ok=True)
    items.sort(key=lambda it: (len(it[1]), it[0]))
    start = time.time()
    frames = samples = 0
    for first in range(0, len(items), jobs):
        batch = items[first:first + jobs]
        mel, en, length = extractor.extract([w for _, w in batch], energy=energy)
        mel, length = mel.cpu().numpy(), length.cpu().tolist()
        en = en.cpu().numpy() if energy else None
        f0 = pitch.extract([w for _, w in batch])[0].cpu().numpy() if pitch is not None else None
        sp = spectrogram.spectrogram([w for _, w in batch])[0].cpu().numpy() if spectrogram is not None else None
        for b, (uid, w) in enumerate(batch):
            T = int(length[b])
            if spectrogram is not None:
                np.save(os.path.join(output_dir, 'spec', uid + '.npy'), np.ascontiguousarray(sp[b, :T], dtype=np.float32))
            if pitch is not None:
                np.save(os.path.join(output_dir, 'pitch', uid + '.npy'), np.ascontiguousarray(f0[b, :T], dtype=np.float32))
            np.save(os.path.join(output_dir, 'mel', uid + '.npy'), np.ascontiguousarray(mel[b, :T], dtype=np.float32))
            if energy:
                np.save(os.path.join(output_dir, 'energy', uid + '.npy'), np.ascontiguousarray(en[b, :T], dtype=np.float32))
            frames, samples = frames + T, samples + len(w)
    took = max(time.time() - start, 1e-9)
    print('%d files, %d frames, %.1f s of audio in %.3f s: %.1f files/s, %.0f frames/s, %.1f audio-seconds/s'
          % (len(items), frames, samples / extractor.sample_rate, took, len(items) / took, frames / took,
             samples / extractor.sample_rate / took), file=out)
    return len(items), frames, samples


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('wav_dir')
    ap.add_argument('-o', '--output-dir', required=True)
    ap.add_argument('--energy', action='store_true', help='also write energy/<id>.npy')
    ap.add_argument('--pitch', action='store_true', help='also write pitch/<id>.npy (YIN log-F0, 0 on unvoiced frames)')
    ap.add_argument('--fmin', type=float, default=None, help='lowest F0 in Hz (default: the config, else 60)')
    ap.add_argument('--fmax', type=float, default=None, help='highest F0 in Hz (default: the config, else 500)')
    ap.add_argument('--threshold', type=float, default=None, help='threshold of YIN (default: the config, else 0.15)')
    ap.add_argument('--spectrogram', action='store_true', help='also write spec/<id>.npy (the normalised linear spectrogram)')
    ap.add_argument('--resample', action='store_true',
                    help='downmix, resample to sample_rate and peak-normalise every file first, in place of refusing other rates')
    ap.add_argument('--norm', default=-7.0, type=lambda v: None if v.lower() == 'none' else float(v),
                    help='with --resample: peak level in dBFS (default -7), or none')
    ap.add_argument('-j', '--jobs', type=int, default=16, help='utterances per launch')
    ap.add_argument('-c', '--config', default=None, help='yaml file with hparams (default: those of the reference)')
    ap.add_argument('--device', default='cuda', help='default: the current GPU')
    args = ap.parse_args(argv)
    if args.jobs < 1:
        ap.error('--jobs must be positive')
    from msmctts_amd.hip.features import FeatureExtractor
    conf = {}
    if args.config is not None:
        import yaml
        with open(args.config) as f:
            conf = yaml.safe_load(f) or {}
    extractor = FeatureExtractor.from_config(conf, device=args.device)
    pitch = None
    if args.pitch:
        from msmctts_amd.hip.pitch import PitchExtractor
        given = {k: getattr(args, k) for k in ('fmin', 'fmax', 'threshold') if getattr(args, k) is not None}
        pitch = PitchExtractor.from_config(conf, device=args.device, **given)
    spectrogram = None
    if args.spectrogram:
        from msmctts_amd.hip.griffin_lim import GriffinLim
        spectrogram = GriffinLim.from_config(conf, device=args.device)
    return extract_dir(extractor, args.wav_dir, args.output_dir, args.energy, args.jobs, pitch=pitch, resample=args.resample,
                       norm_db=args.norm, spectrogram=spectrogram)


if __name__ == '__main__':
    main()
