"""Seeded synthetic batches with the contract of ``MelDataset.collate_fn`` + ``to_model``
(reference msmctts/datasets/mel_dataset.py:25-56, utils/utils.py:137-151).

``mel (B,T,in_dim)`` ~ N(0,1) with padding value -4, ``mel_length (B,) int64`` sorted descending with
``max == T``, ``wav (B, T*hop, 1)`` ~ U(-1,1) with padding 0, ``wav_length = mel_length * hop``.
"""
import torch


def make_batch(batch_size=16, frames=400, in_dim=80, hop=300, seed=1234, rank=0, device='cpu'):
    g = torch.Generator().manual_seed(seed + rank)
    lengths = torch.randint(frames // 2, frames + 1, (batch_size,), generator=g)
    lengths[0] = frames
    lengths = torch.sort(lengths, descending=True).values.to(torch.int64)
    mel = torch.randn(batch_size, frames, in_dim, generator=g)
    wav = torch.rand(batch_size, frames * hop, 1, generator=g) * 2 - 1
    t = torch.arange(frames)[None, :, None]
    mel = torch.where(t < lengths[:, None, None], mel, torch.full_like(mel, -4.0))
    s = torch.arange(frames * hop)[None, :, None]
    wav = torch.where(s < (lengths * hop)[:, None, None], wav, torch.zeros_like(wav))
    batch = {'mel': mel, 'mel_length': lengths, 'wav': wav, 'wav_length': lengths * hop}
    return {k: v.to(device) for k, v in batch.items()}


def make_emb_batch(batch_size=16, frames=400, emb_dim=1024, mel_dim=80, hop=200, seed=1234, rank=0, device='cpu', tracks=False):
    """The contract of ``EmbDataset.collate_fn`` (``EmbVQGANTrainer.train_step``'s batch): ``emb (B,T,emb_dim)`` ~ N(0,1) with
    padding 0, ``emb_length (B,) int64`` sorted descending with ``max == T``, ``mel (B,T,mel_dim)`` ~ N(0,1) with padding -4,
    ``wav (B, T*hop, 1)`` ~ U(-1,1) with padding 0, ``wav_length = emb_length * hop``; ``emb_length_host`` is the host list of
    the lengths the trainer samples its windows from (a loader hands it along; reading ``emb_length`` back would be a sync).
    ``tracks``: also ``pitch`` ~ N(0,1) and ``energy`` ~ U(0,1), (B,T,1) fp32 with padding 0 -- drawn from the same generator after
    everything else, so the other entries keep their bits whatever the flag."""
    g = torch.Generator().manual_seed(seed + rank)
    lengths = torch.randint(frames // 2, frames + 1, (batch_size,), generator=g)
    lengths[0] = frames
    lengths = torch.sort(lengths, descending=True).values.to(torch.int64)
    emb = torch.randn(batch_size, frames, emb_dim, generator=g)
    mel = torch.randn(batch_size, frames, mel_dim, generator=g)
    wav = torch.rand(batch_size, frames * hop, 1, generator=g) * 2 - 1
    valid = torch.arange(frames)[None, :, None] < lengths[:, None, None]
    emb = torch.where(valid, emb, torch.zeros_like(emb))
    mel = torch.where(valid, mel, torch.full_like(mel, -4.0))
    s = torch.arange(frames * hop)[None, :, None]
    wav = torch.where(s < (lengths * hop)[:, None, None], wav, torch.zeros_like(wav))
    batch = {'emb': emb, 'emb_length': lengths, 'mel': mel, 'wav': wav, 'wav_length': lengths * hop}
    if tracks:
        pitch = torch.randn(batch_size, frames, 1, generator=g)
        energy = torch.rand(batch_size, frames, 1, generator=g)
        batch['pitch'] = torch.where(valid, pitch, torch.zeros_like(pitch))
        batch['energy'] = torch.where(valid, energy, torch.zeros_like(energy))
    batch = {k: v.to(device) for k, v in batch.items()}
    batch['emb_length_host'] = lengths.tolist()
    return batch


def make_unit_batch(batch_size=16, frames=400, n_units=1000, mel_dim=80, hop=200, seed=1234, rank=0, device='cpu'):
    """``make_emb_batch`` for stored unit labels (``EmbDataset.collate_fn`` on ``units`` files): ``units (B,T) int64`` uniform in
    [0, n_units) with padding -1 and ``units_length`` in the place of ``emb`` / ``emb_length``; ``mel``, ``wav``, ``wav_length``
    as there; ``units_length_host`` is the host list of the lengths."""
    g = torch.Generator().manual_seed(seed + rank)
    lengths = torch.randint(frames // 2, frames + 1, (batch_size,), generator=g)
    lengths[0] = frames
    lengths = torch.sort(lengths, descending=True).values.to(torch.int64)
    units = torch.randint(0, n_units, (batch_size, frames), generator=g, dtype=torch.int64)
    mel = torch.randn(batch_size, frames, mel_dim, generator=g)
    wav = torch.rand(batch_size, frames * hop, 1, generator=g) * 2 - 1
    valid = torch.arange(frames)[None, :] < lengths[:, None]
    units = torch.where(valid, units, torch.full_like(units, -1))
    mel = torch.where(valid[:, :, None], mel, torch.full_like(mel, -4.0))
    s = torch.arange(frames * hop)[None, :, None]
    wav = torch.where(s < (lengths * hop)[:, None, None], wav, torch.zeros_like(wav))
    batch = {'units': units, 'units_length': lengths, 'mel': mel, 'wav': wav, 'wav_length': lengths * hop}
    batch = {k: v.to(device) for k, v in batch.items()}
    batch['units_length_host'] = lengths.tolist()
    return batch


def make_text_unit_batch(batch_size=16, frames=400, n_units=1000, n_symbols=(100, 10, 2), phonemes=(30, 56), centers=None,
                         seed=1234, rank=0, device='cpu'):
    """A ``UnitPredictorTrainer`` batch: the text side of ``make_text_batch`` (``text``, ``text_length``, ``dur``: durations that
    sum to the utterance's frames) and the unit labels of ``make_unit_batch`` (``units (B,T) int64`` uniform in [0, n_units) with
    padding -1, ``units_length`` sorted descending with ``max == frames``).  With ``centers`` [K, d] (K >= n_units) the batch
    carries the labels' frames instead -- ``emb (B,T,d)`` = the centroid rows of those same labels, zeros on padding, and
    ``emb_length``: the batch a nearest-centroid search turns back into the unit batch."""
    g = torch.Generator().manual_seed(seed + rank)
    lengths = torch.randint(frames // 2, frames + 1, (batch_size,), generator=g)
    lengths[0] = frames
    lengths = torch.sort(lengths, descending=True).values.to(torch.int64)
    units = torch.randint(0, n_units, (batch_size, frames), generator=g, dtype=torch.int64)
    valid = torch.arange(frames)[None, :] < lengths[:, None]
    batch = make_text_batch(lengths.tolist(), n_symbols=n_symbols, phonemes=phonemes, seed=seed + 1, rank=rank)
    if centers is None:
        batch.update(units=torch.where(valid, units, torch.full_like(units, -1)), units_length=lengths)
    else:
        rows = torch.as_tensor(centers, dtype=torch.float32)[units]
        batch.update(emb=torch.where(valid[:, :, None], rows, torch.zeros_like(rows)), emb_length=lengths)
    return {k: v.to(device) for k, v in batch.items()}


def make_text_emb_batch(batch_size=16, frames=400, emb_dim=1024, n_symbols=(100, 10, 2), phonemes=(30, 56), n_codes=None,
                        downsample_scales=(1, 4), n_heads=4, tracks=False, seed=1234, rank=0, device='cpu'):
    """An ``EmbPredictorTrainer`` batch: the text side of ``make_text_batch`` (``text``, ``text_length``, ``dur``: durations that
    sum to the utterance's frames) and, with ``n_codes=None``, frames -- ``emb (B,T,emb_dim)`` ~ N(0,1) with padding 0,
    ``emb_length`` sorted descending with ``max == frames``, and with ``tracks`` also ``pitch`` ~ N(0,1) / ``energy`` ~ U(0,1),
    (B,T,1) with padding 0.  With ``n_codes = K`` the batch carries stored codes instead: ``codes_0 .. codes_{S-1}``, stage 0 the
    coarsest, ``(B, T_i, n_heads) int64`` uniform in [0, K) with padding -1, T_i and the valid lengths from ``frames`` / the
    lengths by ``downsample_scales``' ``ceil`` chain (the finest stage is the frames' own rate when ``downsample_scales[0] == 1``);
    ``codes_length`` the finest stage's lengths, ``codes_length_host`` their host list.  Lengths, text and durations are the same
    in both forms."""
    g = torch.Generator().manual_seed(seed + rank)
    lengths = torch.randint(frames // 2, frames + 1, (batch_size,), generator=g)
    lengths[0] = frames
    lengths = torch.sort(lengths, descending=True).values.to(torch.int64)
    batch = make_text_batch(lengths.tolist(), n_symbols=n_symbols, phonemes=phonemes, seed=seed + 1, rank=rank)
    if n_codes is None:
        valid = torch.arange(frames)[None, :, None] < lengths[:, None, None]
        emb = torch.randn(batch_size, frames, emb_dim, generator=g)
        batch.update(emb=torch.where(valid, emb, torch.zeros_like(emb)), emb_length=lengths)
        if tracks:
            pitch = torch.randn(batch_size, frames, 1, generator=g)
            energy = torch.rand(batch_size, frames, 1, generator=g)
            batch.update(pitch=torch.where(valid, pitch, torch.zeros_like(pitch)),
                         energy=torch.where(valid, energy, torch.zeros_like(energy)))
        return {k: v.to(device) for k, v in batch.items()}
    width, flen, stages = frames, lengths, []
    for i, scale in enumerate(downsample_scales):
        if i > 0 and scale > 1:
            width, flen = -(-width // scale), torch.ceil(flen / scale).long()
        codes = torch.randint(0, n_codes, (batch_size, width, n_heads), generator=g, dtype=torch.int64)
        valid = torch.arange(width)[None, :, None] < flen[:, None, None]
        stages.append(torch.where(valid, codes, torch.full_like(codes, -1)))
    for i, codes in enumerate(stages[::-1]):
        batch['codes_%d' % i] = codes
    batch['codes_length'] = lengths
    batch = {k: v.to(device) for k, v in batch.items()}
    batch['codes_length_host'] = lengths.tolist()
    return batch


def make_text_batch(mel_length, n_symbols=(100, 10, 2), phonemes=(30, 56), seed=4321, rank=0, device='cpu'):
    """The text side of a ``TTSDataset`` batch (reference msmctts/datasets/tts_dataset.py) for the given mel lengths:
    ``text (B, P, 3)`` symbol / tone / boundary ids (0 = padding), ``text_length (B,)``, ``dur (B, P)`` whole-frame durations of
    at least one frame that sum to the utterance's ``mel_length`` -- what the predictor's length regulator expands by."""
    g = torch.Generator().manual_seed(seed + rank)
    lengths = [int(n) for n in mel_length]
    B = len(lengths)
    text_length = torch.randint(phonemes[0], phonemes[1] + 1, (B,), generator=g)
    text_length = torch.minimum(text_length, torch.tensor(lengths)).to(torch.int64)
    P = int(text_length.max())
    text = torch.zeros(B, P, len(n_symbols), dtype=torch.int64)
    dur = torch.zeros(B, P, dtype=torch.int64)
    for b, (tl, ml) in enumerate(zip(text_length.tolist(), lengths)):
        for i, n in enumerate(n_symbols):
            text[b, :tl, i] = torch.randint(1, n, (tl,), generator=g)
        cuts = sorted(torch.randperm(ml - 1, generator=g)[:tl - 1].add(1).tolist())
        edges = [0] + cuts + [ml]
        dur[b, :tl] = torch.tensor([edges[i + 1] - edges[i] for i in range(tl)])
    batch = {'text': text, 'text_length': text_length, 'dur': dur}
    return {k: v.to(device) for k, v in batch.items()}
