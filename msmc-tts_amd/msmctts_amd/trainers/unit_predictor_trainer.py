"""Training a text -> unit predictor against a frozen k-means autoencoder (no reference counterpart: the reference trains its
predictor on the multi-stage quantiser's embeddings, msmctts_trainer.py:222-295, and has no loss for ``KMeansVQGANEmb``).

The predictor is a ``MultiStagePredictor(n_pred_size=K or ceil8(K), n_pred_scale=[1])``: one stage of logits over the K
centroids.  The autoencoder is frozen and must have a frozen codebook (``unit_table``: ``KMeansVQGANEmb``); anything else raises
``TypeError`` at the first step.  The batch is ``text``, ``text_length``, ``dur`` and either stored labels -- ``units`` int64
[B, T] with -1 padding and ``units_length``: no frames are uploaded and no search runs -- or frames, ``emb`` / ``emb_length``,
which ``KMeansQuantizer.units`` labels without a gradient (``synthetic.make_text_unit_batch`` makes both).  The predictor runs
without ``feat`` (one stage: nothing is teacher-forced), the loss is the autoencoder's ``compute_embedding_loss`` with
``training_methods`` (default ``['softmax']``: csrc/unit_ce.hip) plus ``DurationLoss``; clipping and the update are the
parent's.  The class count handed down is the codebook's K whatever the predictor's width.  The loss dictionary also carries
``unit_acc``, the share of valid frames whose arg-max is the label (a device tensor, from the forward kernel's count).

The step is eager: ``use_graphs = True`` raises ``NotImplementedError``.
"""
import torch

from ..hip import norm as hipnorm
from .msmctts_trainer import PredictorTrainer, _one_like


class UnitPredictorTrainer(PredictorTrainer):
    def __init__(self, config, model, num_gpus=1, rank=0, grad_clip_thresh=1.0, eval_inteval_iters=1000,
                 training_methods=['softmax'], loss_weights=[1.0], lambda_dur=1.0):
        super().__init__(config, model, num_gpus, rank, grad_clip_thresh=grad_clip_thresh, eval_inteval_iters=eval_inteval_iters,
                         training_methods=training_methods, loss_weights=loss_weights, lambda_dur=lambda_dur)

    @property
    def use_graphs(self):
        return False

    @use_graphs.setter
    def use_graphs(self, on):
        if on:
            raise NotImplementedError('UnitPredictorTrainer steps eagerly: hipGraph capture of this step is not implemented')

    def _labels(self, batch):
        """(labels [B, T] int64, lengths [B]) of the batch: stored, or the frames' nearest centroids"""
        if 'units' in batch:
            return batch['units'], batch['units_length']
        if 'emb' not in batch:
            raise KeyError('the batch carries neither \'units\' / \'units_length\' nor \'emb\' / \'emb_length\'')
        return self.autoencoder.quantizer.units(batch['emb'], batch['emb_length']), batch['emb_length']

    def _forward_backward(self, batch, static=False):
        ae = self.autoencoder
        if not (hasattr(ae, 'unit_table') and hasattr(ae, 'compute_embedding_loss')):
            raise TypeError('%s has no unit_table: a unit predictor trains against an autoencoder with a frozen codebook, such as '
                            'KMeansVQGANEmb' % type(ae).__name__)
        ae.eval()
        labels, length = self._labels(batch)
        hipnorm.advance_seed(labels.device)          # fresh dropout masks (see PredictorTrainer._forward_backward)
        with self._amp():
            output = self.model.predictor(text=batch['text'], text_length=batch['text_length'], dur=batch['dur'], feat_length=[length])
        logits = output['feat'][0].float()
        if tuple(logits.shape[:2]) != tuple(labels.shape):
            raise ValueError('the durations expand to %s frames, the labels are %s' % (tuple(logits.shape[:2]), tuple(labels.shape)))
        states = {'quantizer_indices': (labels,), 'quantizer_lengths': [length]}
        losses = ae.compute_embedding_loss([logits], [length], states, methods=self.training_methods, loss_weights=self.loss_weights)
        dur = self.dur_loss(output, batch)
        losses['total_loss'] = losses['total_loss'] + dur.pop('total_loss')
        losses.update(dur)
        correct = states.get('unit_correct')         # (left there by the 'softmax' method: the forward kernel's count)
        if correct is None:
            pred = ae.decode_units(logits.detach(), length)
            correct = ((pred == labels) & (pred >= 0)).sum()
        losses['unit_acc'] = correct.float() / length.sum().clamp(min=1)
        self.optimizer.zero_grad(['predictor'])
        losses['total_loss'].backward(gradient=_one_like(losses['total_loss']))
        return losses
