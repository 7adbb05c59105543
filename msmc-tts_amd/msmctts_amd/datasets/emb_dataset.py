"""Speech-embedding dataset of the QS-TTS synthesiser (``dataset._name: EmbDataset`` of examples/qs-tts/configs/synthesizer/
msmc_vq_gan_hubertch_aishell3.yaml).  The reference tree names this class but does not ship it; it is ``MelDataset``'s
collation keyed on ``emb`` -- the batch contract of ``EmbVQGANTrainer.train_step``: utterances sorted by decreasing ``emb``
length, every feature padded with its ``padding_value`` (``emb (B, T, emb_dim)``, ``mel (B, T, mel_dim)``, ``wav (B, T*hop, 1)``,
optional ``pitch`` / ``energy``), one ``<name>_length`` per feature.  A dataset of stored unit labels (``units`` int64 [T], the
``indices/`` files of tools/extract_units.py) without ``emb`` is sorted on ``units``; its padding is ``padding_value['units']``,
which the configuration sets to -1."""
import numpy as np
import torch
from torch.nn.utils.rnn import pad_sequence

from .mel_dataset import MelDataset


class EmbDataset(MelDataset):
    def collate_fn(self, batch):
        cols = {name: [torch.from_numpy(item[name]) if isinstance(item[name], np.ndarray) else item[name] for item in batch]
                for name in batch[0].keys()}
        key = 'units' if 'emb' not in cols and 'units' in cols else 'emb'
        _, order = torch.sort(torch.LongTensor([e.shape[0] for e in cols[key]]), dim=0, descending=True)
        out = {}
        for name, values in cols.items():
            values = [values[i] for i in order]
            if isinstance(values[0], torch.Tensor) and values[0].dim() >= 1:
                out[name + '_length'] = torch.LongTensor([v.shape[0] for v in values])
                values = pad_sequence(values, batch_first=True, padding_value=self.padding_value[name])
            elif isinstance(values[0], torch.Tensor):
                values = torch.stack(values)
            out[name] = values
        return out
