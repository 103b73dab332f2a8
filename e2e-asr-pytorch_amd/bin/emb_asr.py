"""Embedding-fused decoding for the inference Solvers (reference bin/test_asr.py:70-81): when the training config of the
checkpoint has an enabled `emb:` block that fuses (emb.fuse > 0), the plugin of the training run is built, loaded from the
checkpoint's 'emb_decoder' entry and handed to the BeamDecoder.  with_emb_decoder(Solver) wraps bin/test_asr.Solver or
bin/batch_asr.Solver (main.py --test); without such a block the wrapped Solver does exactly what the plain one does."""
from src.decode import BeamDecoder


def with_emb_decoder(solver_cls):
    class Solver(solver_cls):
        def set_model(self):
            emb = self.src_config.get('emb') or {}
            if not (emb.get('enable', False) and emb.get('fuse', 0) > 0):
                return super().set_model()
            from src.plugin import EmbeddingRegularizer
            prec = self.src_config.get('hip', {}).get('prec', 'bf16')
            # built before the model so that load_ckpt (src/solver.py) restores both from the one checkpoint read
            self.emb_decoder = EmbeddingRegularizer(self.tokenizer, self.src_config['model']['decoder']['dim'], prec=prec,
                                                    **emb).to(self.device)
            super().set_model()
            self.emb_decoder.eval()
            kw = dict(self.config['decode'])
            kw['batch_encode'] = self.decoder.batch_encode
            self.decoder = BeamDecoder(self.model, self.emb_decoder, **kw)
            self.verbose(self.decoder.create_msg())

    Solver.__name__, Solver.__qualname__ = solver_cls.__name__, solver_cls.__qualname__
    return Solver
