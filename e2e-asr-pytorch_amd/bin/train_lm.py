"""RNN language-model training Solver (reference bin/train_lm.py:10-123): `fetch_data` (prepend <sos> = 0, lengths), `load_data`,
`set_model`, `exec`, `validate`.  Every tensor op of the step runs in libasr_hip.so: embedding gather / gradient, dropout,
the LSTM stack through the encoder's recurrence kernels or the GRU stack through gru_rec.hip, the output projection, cross entropy,
clip + Adam."""
import torch

from src import hipabi as H
from src.data import load_textset
from src.lm import RNNLM
from src.optim import Optimizer
from src.solver import BaseSolver
from src.util import CrossEntropyLoss, human_format


class Solver(BaseSolver):
    def __init__(self, config, paras, mode):
        super().__init__(config, paras, mode)
        self.best_loss = 10

    def fetch_data(self, data):
        txt = torch.cat((torch.zeros((data.shape[0], 1), dtype=torch.long), data), dim=1).to(self.device)
        txt_len = torch.sum(data != 0, dim=-1)
        return txt, txt_len

    def load_data(self):
        self.tr_set, self.dv_set, self.vocab_size, self.tokenizer, msg = \
            load_textset(self.paras.njobs, self.paras.gpu, self.paras.pin_memory, **self.config['data'])
        self.verbose(msg)

    def set_model(self):
        self.model = RNNLM(self.vocab_size, **self.config['model']).to(self.device)
        self.model.prec = H.BF16 if self.config.get('hip', {}).get('prec', 'bf16') == 'bf16' else H.F32
        self.model.flatten()              # flat parameter / gradient storage for the fused optimizer (after the move to the device)
        self.verbose(self.model.create_msg())
        self.seq_loss = CrossEntropyLoss(ignore_index=0)
        self.optimizer = Optimizer(self.model.parameters(), **self.config['hparas'])
        self.verbose(self.optimizer.create_msg())
        self.load_ckpt()

    def _loss(self, txt, txt_len):
        pred, _ = self.model(txt[:, :-1], txt_len)
        return pred, self.seq_loss(pred.view(-1, self.vocab_size), txt[:, 1:].reshape(-1))

    def exec(self):
        self.verbose('Total training steps {}.'.format(human_format(self.max_step)))
        self.timer.set()
        while self.step < self.max_step:
            for data in self.tr_set:
                self.optimizer.pre_step(self.step)
                txt, txt_len = self.fetch_data(data)
                self.timer.cnt('rd')
                pred, lm_loss = self._loss(txt, txt_len)
                self.timer.cnt('fw')
                grad_norm = self.backward(lm_loss)
                self.step += 1
                if self.step % self.PROGRESS_STEP == 0:
                    H.raise_if_aborted()
                    self.progress('Tr stat | Loss - {:.2f} | Grad. Norm - {:.2f} | {}'.format(
                        lm_loss.item(), grad_norm.item(), self.timer.show()))
                    self.write_log('entropy', {'tr': lm_loss})
                    self.write_log('perplexity', {'tr': torch.exp(lm_loss.detach()).item()})
                if (self.step == 1) or (self.step % self.valid_step == 0):
                    self.validate()
                self.timer.set()
                if self.step >= self.max_step:
                    break
        self.log.close()

    def validate(self):
        self.model.eval()
        dev_loss = []
        txt, pred = None, None
        for i, data in enumerate(self.dv_set):
            self.progress('Valid step - {}/{}'.format(i + 1, len(self.dv_set)))
            txt, txt_len = self.fetch_data(data)
            with torch.no_grad():
                pred, lm_loss = self._loss(txt, txt_len)
            dev_loss.append(lm_loss)
        dev_loss = sum(dev_loss) / len(dev_loss)
        dev_ppx = torch.exp(dev_loss).item()
        if dev_loss < self.best_loss:
            self.best_loss = dev_loss
            self.save_checkpoint('best_ppx.pth', 'perplexity', dev_ppx)
        self.write_log('entropy', {'dv': dev_loss})
        self.write_log('perplexity', {'dv': dev_ppx})
        for i in range(min(len(txt), self.DEV_N_EXAMPLE)):
            if self.step == 1:
                self.write_log('true_text{}'.format(i), self.tokenizer.decode(txt[i].tolist()))
            self.write_log('pred_text{}'.format(i), self.tokenizer.decode(pred[i].argmax(dim=-1).tolist()))
        self.model.train()
