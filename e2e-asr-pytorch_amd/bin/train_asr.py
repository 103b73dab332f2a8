"""Training Solver with the reference's surface (bin/train_asr.py:17-394): `load_data`, `set_model`, `exec`,
`fetch_data`, `validate`.  The step is src/step.py's: forward_losses here, backward_update in BaseSolver.backward."""
import torch

from src import hipabi as H
from src.asr import ASR
from src.data import load_dataset
from src.optim import Optimizer
from src.solver import BaseSolver
from src.step import forward_losses
from src.util import human_format, cal_er, CTCLoss, CrossEntropyLoss, LabelSmoothingLoss


class Solver(BaseSolver):
    def __init__(self, config, paras, mode):
        super().__init__(config, paras, mode)
        self.curriculum = self.config['hparas'].get('curriculum', 0)
        self.val_mode = self.config['hparas'].get('val_mode', 'wer').lower()
        self.WER = 'per' if self.val_mode == 'per' else 'wer'

    def fetch_data(self, data, train=False):
        """Batch to the device; a WAVEFORM batch (B,N) goes through the GPU front-end here - fbank, delta stack and, in
        training, SpecAugment - which the reference runs per utterance on the CPU inside its DataLoader workers
        (src/audio.py:453-486, src/collect_batch.py:32)."""
        _, feat, feat_len, txt = data
        feat, feat_len, txt = feat.to(self.device), feat_len.to(self.device), txt.to(self.device)
        if feat.dim() == 2:
            tf = (self.tr_set if train else self.dv_set).audio_transform
            with torch.no_grad():
                feat, feat_len = tf(feat, feat_len)
        return feat, feat_len, txt, torch.sum(txt != 0, dim=-1)

    def load_data(self):
        audio = dict(self.config['data']['audio'])
        audio.setdefault('time_aug', False)          # omitted by config/librispeech_asr.yaml
        self.tr_set, self.dv_set, self.feat_dim, self.vocab_size, self.tokenizer, msg = load_dataset(
            self.paras.njobs, self.paras.gpu, self.paras.pin_memory, self.curriculum > 0,
            self.config['data']['corpus'], audio, self.config['data']['text'], rank=self.rank, world=self.world)
        self.verbose(msg)
        for ld in (self.tr_set, self.dv_set):
            if getattr(ld, 'audio_transform', None) is not None:
                ld.audio_transform = ld.audio_transform.to(self.device)
        self.dv_names = self.config['data']['corpus']['dev_split'][0]
        self.best_wer = {'att': {self.dv_names: 3.0}, 'ctc': {self.dv_names: 3.0}}

    def set_model(self):
        hip = self.config.get('hip', {})
        batch_size = self.config['data']['corpus']['batch_size'] // 2
        self.model = ASR(self.feat_dim, self.vocab_size, batch_size, prec=hip.get('prec', 'bf16'),
                         seed=self.paras.seed + 7919 * self.rank, **self.config['model']).to(self.device)
        self.verbose(self.model.create_msg())
        hp = dict(self.config['hparas'])
        if hp.get('label_smoothing', False):        # default False when the YAML omits it
            self.seq_loss = LabelSmoothingLoss(31, 0.1)
        else:
            self.seq_loss = CrossEntropyLoss(ignore_index=0)
        self.ctc_loss = CTCLoss(blank=0, zero_infinity=False)
        self.optimizer = Optimizer(self.model.parameters(), **hp)
        self.lr_scheduler = self.optimizer.lr_scheduler
        self.verbose(self.optimizer.create_msg())
        # word-embedding regulariser (reference bin/train_asr.py:139-147).  Its parameters get an optimizer of the same kind beside
        # the model's: the fused step kernels work on one flat buffer each (src/step.step_emb_optimizer)
        self.emb_fuse, self.emb_reg = False, ('emb' in self.config) and self.config['emb'].get('enable', False)
        if self.emb_reg:
            from src.plugin import EmbeddingRegularizer, check_emb_config
            check_emb_config(self.config['emb'], self.config['model'], hp)
            if torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
                raise NotImplementedError('the embedding regulariser is not wired into data-parallel training (its gradients are '
                                          'not all-reduced)')
            self.emb_decoder = EmbeddingRegularizer(self.tokenizer, self.model.dec_dim, prec=hip.get('prec', 'bf16'),
                                                    seed=self.paras.seed, **self.config['emb']).to(self.device)
            self.emb_optimizer = Optimizer(self.emb_decoder.trainable_parameters(), **hp)
            self.emb_fuse = self.emb_decoder.apply_fuse
            self.verbose(self.emb_decoder.create_msg())
        from src import dist as D_
        if torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
            self.dp = self.model.attach_data_parallel()
            self.dp.broadcast_params(0)
        self.load_ckpt()

    def exec(self):
        # single-process runs overlap the parameter gradients with the BPTT on CU-masked streams, which serialise against
        # the legacy default stream (src/hipabi.work_stream): the whole loop runs on a non-default stream then
        if H.step_overlaps(self.dp) and torch.cuda.is_available():
            with H.on_work_stream():       # behind model init / flatten / broadcast / load_ckpt, which ran on the default stream
                self._exec()
        else:
            self._exec()

    def _exec(self):
        self.verbose('Total training steps {}.'.format(human_format(self.max_step)))
        self.timer.set()
        while self.step < self.max_step:
            for data in self.tr_set:
                tf_rate = self.optimizer.pre_step(self.step)      # zeroes the model's gradient
                if self.emb_reg:
                    self.emb_decoder.zero_grad()
                feat, feat_len, txt, txt_len = self.fetch_data(data, train=True)
                self.timer.cnt('rd')
                L = int(txt.shape[1])      # = max(txt_len) for a padded batch, without a device sync
                out = forward_losses(self.model, self.ctc_loss, self.seq_loss, feat, feat_len, txt, L, tf_rate, self.dp, txt_len, self.emb_decoder)
                self.timer.cnt('fw')
                grad_norm = self.backward(out['total_loss'])
                self.step += 1
                if (self.step == 1) or (self.step % self.PROGRESS_STEP == 0):
                    H.raise_if_aborted()      # the host synchronises here anyway (loss.item()): surface a refused step
                    self.progress('Tr stat | Loss - {:.2f} | Grad. Norm - {:.2f} | {}'.format(
                        out['total_loss'].item(), grad_norm.item(), self.timer.show()))
                    if out['att_output'] is not None:
                        self.write_log('loss', {'tr_att': out['att_loss']})
                        self.write_log(self.WER, {'tr_att': cal_er(self.tokenizer, out['att_output'], txt)})
                    if out['ctc_output'] is not None:
                        self.write_log('loss', {'tr_ctc': out['ctc_loss']})
                        self.write_log(self.WER, {'tr_ctc': cal_er(self.tokenizer, out['ctc_output'], txt, ctc=True)})
                    if self.emb_reg:
                        self.write_log('emb_loss', {'tr': out['emb_loss']})
                        if self.emb_fuse:
                            if self.emb_decoder.fuse_learnable:
                                self.write_log('fuse_lambda', {'emb': self.emb_decoder.get_weight()})
                            self.write_log('fuse_temp', {'temp': self.emb_decoder.get_temp()})
                if (self.step == 1) or (self.step % self.valid_step == 0):
                    self.validate(self.dv_set, self.dv_names)
                if self.lr_scheduler is None and self.step > 99999 and self.step % 2000 == 0:
                    for g in self.optimizer.opt.param_groups:      # hand-rolled decay, bin/train_asr.py:292-303
                        g['lr'] = g['lr'] * 0.85
                self.timer.set()
                if self.step >= self.max_step:
                    break
        self.log.close()
        print('[INFO] Finished training after', human_format(self.max_step), 'steps.')

    def validate(self, _dv_set, _name):
        self.model.eval()
        if self.emb_decoder is not None:
            self.emb_decoder.eval()
        dev_er = {'att': [], 'ctc': []}
        for i, data in enumerate(_dv_set):
            self.progress('Valid step - {}/{}'.format(i + 1, len(_dv_set)))
            feat, feat_len, txt, txt_len = self.fetch_data(data)
            with torch.no_grad():
                ctc_output, encode_len, att_output, att_align, _ = self.model(
                    feat, feat_len, int(txt.shape[1] * self.DEV_STEP_RATIO), emb_decoder=self.emb_decoder)
            if att_output is not None:
                dev_er['att'].append(cal_er(self.tokenizer, att_output, txt, mode=self.val_mode))
            if ctc_output is not None:
                dev_er['ctc'].append(cal_er(self.tokenizer, ctc_output, txt, mode=self.val_mode, ctc=True))
        H.raise_if_aborted()
        for task in [k for k, v in dev_er.items() if len(v) > 0]:
            er = sum(dev_er[task]) / len(dev_er[task])
            if er < self.best_wer[task][_name]:
                self.best_wer[task][_name] = er
                self.save_checkpoint('best_{}_{}.pth'.format(task, _name), self.val_mode, er, _name)
            if self.step >= self.max_step:
                self.save_checkpoint('last_{}_{}.pth'.format(task, _name), self.val_mode, er, _name)
            self.write_log(self.WER, {'dv_' + task + '_' + _name.lower(): er})
        self.model.train()
        if self.emb_decoder is not None:
            self.emb_decoder.train()
