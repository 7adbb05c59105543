"""Training step of the QS-TTS synthesiser ``MSMCVQGANEmb`` (re-expression of reference
msmctts/trainers/emb_vqgan_trainer.py:15-172; configuration examples/qs-tts/configs/synthesizer/
msmc_vq_gan_hubertch_aishell3.yaml, ``trainer._name: EmbVQGANTrainer``).

What differs from ``VQGANTrainer``:

* the batch carries speech-embedding frames ``emb`` / ``emb_length`` next to ``mel`` (the frame-loss target and, with a
  ``global_encoder``, the reference utterance) and optional ``pitch`` / ``energy`` tracks; ``mel_length`` IS ``emb_length``;
* ``sample_batch_size`` of the batch's utterances are decoded to waveform, one window of ``sample_lengths`` samples each
  (:41-56).  The (utterance, start frame) pairs go to the device once as an int32 table and both window sets -- the
  vocoder's input frames inside the model and the target waveform here -- are cut by hip/window.py's ``window_gather``;
* three phases by iteration: no vocoder while ``iteration <= frame_loss_supervised_step``; then vocoder + spectral loss (the
  spectral loss is on whenever the vocoder runs, :84-94); adversarial terms once ``iteration > stft_loss_supervised_step``.

Losses, their weights, the loss-dictionary keys, the discriminator and generator steps, clipping and the optimizer order are
the parent's (the fused loss kernels, the single D([fake; real]) pass, the front-end reuse, the side branches).

A task whose autoencoder is ``KMeansVQGANEmb`` trains here as well, in all three phases.  That model returns
``encoder_indices`` but no ``encoder_diffs`` (its codebook is frozen and its input is data: a VQ term could train nothing), on
which the reference's step fails with a ``KeyError``; here a model output without ``encoder_diffs`` takes no VQ term and the
loss dictionary carries no VQ keys (one guarded branch in ``VQGANTrainer._segment_a``).  Outputs that have ``encoder_diffs``
behave as before.  ``EmbVC`` -- no quantiser: neither ``encoder_diffs`` nor ``encoder_indices`` -- takes the same branch; nothing in
the step reads ``encoder_indices``.

A batch of stored unit labels -- ``units`` int64 [B, T] with -1 padding and ``units_length`` in the place of ``emb`` /
``emb_length`` (``EmbDataset`` on ``indices/`` files, ``synthetic.make_unit_batch``) -- goes to the model's ``forward_units``
(``KMeansVQGANEmb``: no frames uploaded, no centroid search); a model without one raises ``TypeError``.  A batch with ``emb``
behaves as before.

``stft_loss_supervised_step``: the reference reads ``self.stft_loss_supervised_step`` (:123) but no constructor sets it, and
its own YAML passes it as a trainer kwarg (line 94) that its constructor would reject; here it is an ordinary kwarg.

Refused at construction: ``stft_loss_supervised_step < frame_loss_supervised_step`` (the reference would reach the
discriminator without a prediction: a NameError there, a ``ValueError`` here); a task with a ``prosody_estimator`` child
(:97-120 -- the reference ships no such network): ``NotImplementedError``.  ``use_graphs = True`` raises
``NotImplementedError``: this step is not captured into hipGraphs.
"""
import torch

from ..hip import window as hipwindow
from .msmctts_trainer import VQGANTrainer, _StepState


class EmbVQGANTrainer(VQGANTrainer):
    def __init__(self, *args, sample_batch_size=-1, frame_loss_supervised_step=0, stft_loss_supervised_step=0, **kwargs):
        super().__init__(*args, **kwargs)
        if stft_loss_supervised_step < frame_loss_supervised_step:
            raise ValueError('stft_loss_supervised_step (%d) < frame_loss_supervised_step (%d): the adversarial terms would '
                             'start before the vocoder runs' % (stft_loss_supervised_step, frame_loss_supervised_step))
        if hasattr(self.model, 'prosody_estimator'):
            raise NotImplementedError('EmbVQGANTrainer: the adversarial prosody-estimator branch is not implemented')
        if self.frame_lengths < 1:
            raise ValueError('sample_lengths (%r) must cover at least one frame of %d samples' % (self.sample_lengths,
                                                                                                  self.frameshift))
        self.sample_batch_size = sample_batch_size
        self.frame_loss_supervised_step = frame_loss_supervised_step
        self.stft_loss_supervised_step = stft_loss_supervised_step

    @property
    def use_graphs(self):
        return False

    @use_graphs.setter
    def use_graphs(self, on):
        if on:
            raise NotImplementedError('EmbVQGANTrainer steps eagerly: hipGraph capture of this step is not implemented')

    def _phase(self, iteration):
        """0 = frames only (no vocoder), 1 = vocoder + spectral loss, 2 = 1 + adversarial terms"""
        if iteration <= self.frame_loss_supervised_step:
            return 0
        return 2 if iteration > self.stft_loss_supervised_step else 1

    def _spectral_on(self, st):
        return st.phase > 0

    def sample_windows(self, lengths):
        """-> [(utterance, start frame)]: the reference's draws in its order (:41-53) -- shuffle range(B), keep the first
        ``sample_batch_size``, sort (only when ``sample_batch_size > 0``), then one start per kept utterance"""
        seq = list(range(len(lengths)))
        if self.sample_batch_size > 0:
            self.rng.shuffle(seq)
            seq = sorted(seq[:self.sample_batch_size])
        return [(i, self.rng.randrange(max(1, int(lengths[i]) - self.frame_lengths))) for i in seq]

    @staticmethod
    def _frames_key(batch):
        """'emb', or 'units' for a batch of stored unit labels (``units`` int64 [B, T] with -1 padding, ``units_length``) that
        carries no ``emb``: the feature whose ``<key>_length`` / ``<key>_length_host`` are the frame lengths and whose device is
        the step's"""
        return 'units' if 'emb' not in batch and 'units' in batch else 'emb'

    def _autoencode(self, st):
        b = st.batch
        window_frames = None if st.frame_window is None else self.frame_lengths
        if self._frames_key(b) == 'units':
            model = self.model.autoencoder
            if not hasattr(model, 'forward_units'):
                raise TypeError('%s has no forward_units: a batch of unit labels (\'units\' without \'emb\') needs a model with a '
                                'frozen codebook, such as KMeansVQGANEmb' % type(model).__name__)
            return model.forward_units(b['units'], st.mel_length, mel=st.mel, window=st.frame_window, window_frames=window_frames)
        # (no ``ref``: a model with a global encoder embeds ``mel``)
        return self.model.autoencoder(b['emb'], st.mel_length, b.get('pitch'), b.get('energy'), mel=st.mel,
                                      window=st.frame_window, window_frames=window_frames)

    def _target(self, wav, pairs, win):
        """the waveform windows [n, frame_lengths * frameshift] fp32 at ``start * frameshift``"""
        B, hop, fl = wav.shape[0], self.frameshift, self.frame_lengths
        wav = wav.reshape(B, -1)
        if wav.shape[1] % hop == 0:           # rows of ``hop`` samples: the frame table addresses them as it stands
            out = hipwindow.window_gather(wav.reshape(B, -1, hop), win, fl, torch.float32)
        else:
            out = hipwindow.window_gather(wav.unsqueeze(-1), [(i, s * hop) for i, s in pairs], fl * hop, torch.float32)
        return out.reshape(len(pairs), fl * hop)

    def train_step(self, batch, iteration):
        phase = self._phase(iteration)
        reducer = getattr(self.model, 'grad_reducer', None)
        if reducer is not None:
            reducer.hooks_enabled = True
        st = _StepState()
        key = self._frames_key(batch)
        st.phase, st.batch, st.mel, st.mel_length = phase, batch, batch['mel'], batch[key + '_length']
        st.frame_window = st.target = None
        if phase > 0:
            lengths = batch.get(key + '_length_host')
            if lengths is None:
                lengths = batch[key + '_length'].tolist()
            st.windows = pairs = self.sample_windows(lengths)
            st.frame_window = hipwindow.as_windows(pairs, batch[key].device)
            st.target = self._target(batch['wav'].float(), pairs, st.frame_window)
        self._segment_a(st)
        self._sync_codebooks()
        if phase == 2:
            self._sync_grads()
        self._segment_b(st)
        self._sync_grads()
        self._segment_c(st)
        self.last_windows = getattr(st, 'windows', None)
        return {'loss': {k: (v.detach() if torch.is_tensor(v) else v) for k, v in st.losses.items()}}
