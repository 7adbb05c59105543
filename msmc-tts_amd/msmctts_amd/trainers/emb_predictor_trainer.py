"""Training the text front-end of the QS-TTS synthesiser: a ``MultiStagePredictor`` against a frozen ``MSMCVQGANEmb``
(re-expression of reference msmctts/trainers/emb_vqgan_trainer.py:177-252, ``NASynEmbFSTrainer``; configuration
examples/qs-tts/configs/predictor/msmc_vq_gan_hubertch_aishell3_dec_null_tts_15m.yaml).  ``NASynEmbFSTrainer`` below is the same
class under the reference's name, so that YAML's ``trainer._name`` resolves.

The step is the reference's (:192-243): the frozen autoencoder in eval mode under ``no_grad`` turns the batch into per-stage
quantised targets, the predictor maps ``text`` / ``text_length`` / ``dur`` to those stages with the targets as teacher-forcing
inputs (``feat`` / ``feat_length``), the loss is the autoencoder's ``compute_embedding_loss`` (``training_methods``,
``loss_weights``) plus the duration loss; clipping and the update are ``PredictorTrainer``'s.  The reference's ``FSLoss`` comes
from a module it does not ship (``fastspeech_trainer``, :176); ``DurationLoss`` -- the masked duration MSE the predictor trainer of
the mel model uses (reference msmctts_trainer.py:12-36) -- stands in for it, as in ``PredictorTrainer``.  The dropout seed of the
fused kernels advances once per step, as there.

The batch takes one of two forms (``synthetic.make_text_emb_batch`` makes both):

* frames -- ``emb`` / ``emb_length`` and optional ``pitch`` / ``energy``: the targets are
  ``autoencoder.analysis(emb, emb_length.int(), pitch=, energy=)``, as in the reference;
* stored codes (no reference counterpart) -- ``codes_0 .. codes_{S-1}``, stage 0 the coarsest, integer [B, T_i, H] with -1
  padding (a single-head stage also [B, T_i]), as ``tools/extract_codes.py`` writes them, with ``codes_length`` (the finest
  stage's lengths) and optionally ``codes_length_host``.  The per-stage lengths follow from ``codes_length`` and the
  autoencoder's ``downsample_scales`` by the ``ceil`` chain of ``MAMSEncoder``; the targets are
  ``autoencoder.analysis_codes``: one gather per stage (csrc/code_embed.hip).  No frames are uploaded, no encoder and no search
  runs.  The targets are the code rows themselves where ``analysis`` returns them up to two roundings (see the module docstring of
  networks/vqgantts/msmc_vqgan_emb.py).

With both forms in one batch the frames win (as ``EmbVQGANTrainer._frames_key``).  Refused: a code batch for an autoencoder without
``analysis_codes`` (``TypeError``); a number of code tensors other than the number of stages, or a code width other than the
stage's head count (``ValueError``); ``use_graphs = True`` (``NotImplementedError``: the step is eager).
"""
import torch

from ..hip import norm as hipnorm
from .msmctts_trainer import PredictorTrainer, _one_like


class EmbPredictorTrainer(PredictorTrainer):
    def __init__(self, config, model, num_gpus=1, rank=0, grad_clip_thresh=1.0, eval_inteval_iters=1000,
                 training_methods=['mse'], loss_weights=[1.0], lambda_dur=1.0):
        super().__init__(config, model, num_gpus, rank, grad_clip_thresh=grad_clip_thresh, eval_inteval_iters=eval_inteval_iters,
                         training_methods=training_methods, loss_weights=loss_weights, lambda_dur=lambda_dur)

    @property
    def use_graphs(self):
        return False

    @use_graphs.setter
    def use_graphs(self, on):
        if on:
            raise NotImplementedError('EmbPredictorTrainer steps eagerly: hipGraph capture of this step is not implemented')

    @staticmethod
    def _code_keys(batch):
        """'codes_0', 'codes_1', ... in stage order"""
        keys = [k for k in batch if k.startswith('codes_') and k[6:].isdigit()]
        return sorted(keys, key=lambda k: int(k[6:]))

    def stage_lengths(self, codes_length):
        """the per-stage lengths, coarse to fine, from the finest stage's: ``MAMSEncoder.forward``'s chain"""
        ae = self.autoencoder
        scales = list(getattr(ae.encoder, 'downsample_scales', None) or ae.quantizer.upsample_scales[::-1])
        flen = codes_length.int()
        lengths = [flen]
        for scale in scales[1:]:
            if scale > 1:
                flen = torch.ceil(flen / scale).int()
            lengths.append(flen)
        return lengths[::-1]

    def _targets(self, batch):
        """the quantiser's states of the batch: from frames through ``analysis``, from stored codes through ``analysis_codes``"""
        ae = self.autoencoder
        if 'emb' in batch:
            return ae.analysis(batch['emb'], batch['emb_length'].int(), pitch=batch.get('pitch'), energy=batch.get('energy'))
        keys = self._code_keys(batch)
        if not keys:
            raise KeyError('the batch carries neither \'emb\' / \'emb_length\' nor \'codes_<i>\' / \'codes_length\'')
        if not hasattr(ae, 'analysis_codes'):
            raise TypeError('%s has no analysis_codes: a batch of stored codes (\'codes_<i>\' without \'emb\') needs a multi-stage '
                            'autoencoder such as MSMCVQGANEmb' % type(ae).__name__)
        stages = len(ae.quantizer.quantizer)
        if len(keys) != stages or keys != ['codes_%d' % i for i in range(stages)]:
            raise ValueError('the batch carries %s, the autoencoder has %d stages' % (keys, stages))
        codes = []
        for i, k in enumerate(keys):
            c, heads = batch[k], getattr(ae.quantizer.quantizer[i], 'n_head', 1)
            if (c.shape[-1] if c.dim() == 3 else 1 if c.dim() == 2 else -1) != heads:
                raise ValueError('%s is %s: stage %d has %d heads' % (k, tuple(c.shape), i, heads))
            c = c.long()                          # (what the loss kernels take; a no-op on int64)
            codes.append(c.squeeze(-1) if heads == 1 and c.dim() == 3 else c)        # ... in the shape ``analysis`` returns them
        return ae.analysis_codes(tuple(codes), self.stage_lengths(batch['codes_length']))

    def _forward_backward(self, batch, static=False):
        ae = self.autoencoder
        ae.eval()
        with torch.no_grad():
            qs = self._targets(batch)
        feed = {k: batch[k] for k in ('text', 'text_length', 'dur') if k in batch}
        feed['feat'] =[f.float() for f in qs['quantizer_outputs']]
        feed['feat_length'] = qs['quantizer_lengths']
        hipnorm.advance_seed(feed['feat'][0].device)          # fresh dropout masks (see PredictorTrainer._forward_backward)
        with self._amp():
            output = self.model.predictor(**feed)
        output['feat'] = [f.float() for f in output['feat']]
        losses = {'total_loss': 0}
        emb = ae.compute_embedding_loss(output['feat'], output['feat_length'], qs, methods=self.training_methods,
                                        loss_weights=self.loss_weights)
        losses['total_loss'] = losses['total_loss'] + emb.pop('total_loss')
        losses.update(emb)
        dur = self.dur_loss(output, batch)
        losses['total_loss'] = losses['total_loss'] + dur.pop('total_loss')
        losses.update(dur)
        self.optimizer.zero_grad(['predictor'])
        losses['total_loss'].backward(gradient=_one_like(losses['total_loss']))
        return losses


NASynEmbFSTrainer = EmbPredictorTrainer
