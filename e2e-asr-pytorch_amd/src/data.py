"""Batch sources with the reference's contract (src/data.py:104-143, src/collect_batch.py:10-48,
corpus/preprocess_librispeech.py:36-93).

Two kinds of corpus:

* WAVEFORM SHARDS ON DISK (`corpus.path` = a directory).  FLAC decoding is outside this build (no codec offline), so
  the corpus is read from pre-decoded waveforms: `<path>/<split>/manifest.tsv` with one line per utterance
  `utt_id <TAB> file <TAB> n_samples <TAB> transcript`, `file` a .npy of float32 (or int16 PCM) samples relative to the
  split directory (tools/make_waveform_shards.py writes this layout).  The dataset follows the reference:
  utterances sorted by length, longest first (the reference sorts by file size, `preprocess_librispeech.py:69-75`);
  with bucketing `__getitem__(i)` returns the bucket of `bucket_size` neighbours starting at `min(len - bucket, i)`
  (`:83-88`) and the DataLoader shuffles bucket starts; the collate halves a training batch whose longest utterance
  exceeds 800 frames (`collect_batch.py:21-24`) and zero-pads.  What changes: the collate pads WAVEFORMS (B,N), and the
  reference's per-utterance CPU transform (fbank -> delta -> SpecAugment in DataLoader workers, `src/audio.py:453-486`)
  runs batched on the GPU inside `Solver.fetch_data` through `loader.audio_transform` (src/audio.create_transform).
  Under data parallelism rank r takes every world-th bucket (whole utterances are sharded).

* SYNTHETIC (`corpus.path: 'synthetic'` features, `'synthetic-wav'` waveforms): LibriSpeech-shaped random batches with
  the same bucketing / halving behaviour, for benchmarks and plumbing tests (no corpus is available offline).

Every loader yields (names, x, x_len, txt): x = features (B,T,D) or waveforms (B,N) fp32 zero-padded, lengths int64
descending, txt (B,L) int64 0-padded, each row ending in <eos>=1.
"""
import os

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset

from src.synthetic import librispeech_shaped_batch
from src.text import load_text_encoder

HALF_BATCHSIZE_AUDIO_LEN = 800      # frames (reference src/collect_batch.py:6)
HOP = 160                           # samples per frame: frame_shift 10 ms at the nominal 16 kHz (src/audio.py:133)


class SyntheticLoader(object):
    def __init__(self, n_batches, batch_size, feat_dim, vocab_size, seed, train, max_frames=2450, waveform=False):
        self.n, self.bs, self.D, self.V, self.seed, self.train, self.maxT = n_batches, batch_size, feat_dim, vocab_size, seed, train, max_frames
        self.waveform = waveform
        self.audio_transform = None

    def __len__(self):
        return self.n * self.bs

    def __iter__(self):
        g = np.random.Generator(np.random.PCG64(self.seed))
        for i in range(self.n):
            T = int(np.clip(round(g.normal(1270, 480)), 150, self.maxT))
            B = max(1, self.bs // 2) if (self.train and T > HALF_BATCHSIZE_AUDIO_LEN) else self.bs
            L = int(np.clip(round(T * 0.14), 5, 400))
            feat, flen, txt = librispeech_shaped_batch(B, T, 1 if self.waveform else self.D, L, self.V, seed=self.seed * 7919 + i)
            names = ['synthetic-%d-%d' % (i, b) for b in range(B)]
            if self.waveform:
                # waveform batch whose frame counts are the drawn lengths: N = (T - 1) * hop + 1 samples
                g2 = np.random.Generator(np.random.PCG64(self.seed * 104729 + i))
                wlen = (flen - 1) * HOP + 1
                wav = torch.zeros(B, int(wlen.max()))
                for b in range(B):
                    n = int(wlen[b])
                    t = np.arange(n) / 16000.0
                    f0 = 120.0 + 40.0 * b
                    sig = 0.2 * np.sin(2 * np.pi * f0 * t) + 0.1 * np.sin(2 * np.pi * 3.1 * f0 * t) + 0.02 * g2.standard_normal(n)
                    wav[b, :n] = torch.from_numpy(sig.astype(np.float32))
                yield names, wav, wlen, txt
            else:
                yield names, feat, flen, txt


class WaveformShardDataset(Dataset):
    """Pre-decoded LibriSpeech-style corpus (see the module docstring); mirrors LibriDataset of the reference."""

    def __init__(self, path, split, tokenizer, bucket_size=1, ascending=False, subset=None):
        self.bucket_size = bucket_size
        items = []
        for s in split:
            sdir = os.path.join(path, s)
            man = os.path.join(sdir, 'manifest.tsv')
            assert os.path.isfile(man), 'No data found @ {}'.format(man)
            with open(man, 'r', encoding='utf-8') as f:
                for line in f:
                    cols = line.rstrip('\n').split('\t')
                    if len(cols) < 4:
                        continue
                    items.append((int(cols[2]), os.path.join(sdir, cols[1]), cols[0], tokenizer.encode(cols[3])))
        assert len(items) > 0, 'No data found @ {}'.format(path)
        if type(subset) is int:
            items = items[:subset]
        items.sort(key=lambda x: x[0], reverse=not ascending)
        self.n_samples = [it[0] for it in items]
        self.file_list = [it[1] for it in items]
        self.names = [it[2] for it in items]
        self.text = [it[3] for it in items]

    def _item(self, i):
        return self.file_list[i], self.text[i], self.n_samples[i], self.names[i]

    def __getitem__(self, index):
        if self.bucket_size > 1:
            index = min(len(self.file_list) - self.bucket_size, index)
            index = max(index, 0)
            return [self._item(i) for i in range(index, min(index + self.bucket_size, len(self.file_list)))]
        return self._item(index)

    def __len__(self):
        return len(self.file_list)


def read_waveform(path):
    w = np.load(path, mmap_mode='r')
    if w.dtype == np.int16:
        return torch.from_numpy(np.array(w, dtype=np.float32) / 32768.0)
    return torch.from_numpy(np.array(w, dtype=np.float32))


def collect_wav_batch(batch, mode):
    """list of (file, tokens, n_samples, name) or [bucket] -> (names, wav (B,N), wav_len (B), txt (B,L));
    the halving rule of collect_audio_batch (src/collect_batch.py:21-24) on the frame count of the first = longest item."""
    if type(batch[0]) is not tuple:
        batch = batch[0]
    if mode == 'train':
        first_frames = 1 + (batch[0][2] - 1) // HOP
        if first_frames > HALF_BATCHSIZE_AUDIO_LEN:
            batch = batch[::2]
    wavs = [read_waveform(b[0]).reshape(-1) for b in batch]
    lens = torch.LongTensor([len(w) for w in wavs])
    wav = torch.nn.utils.rnn.pad_sequence(wavs, batch_first=True)
    txt = torch.nn.utils.rnn.pad_sequence([torch.LongTensor(b[1]) for b in batch], batch_first=True)
    return [b[3] for b in batch], wav, lens, txt


class _RankShard(torch.utils.data.Sampler):
    """Every world-th index (bucket start) of a seeded permutation: whole utterances are sharded over the ranks and every
    rank takes the same number of steps per epoch (the tail is dropped)."""

    def __init__(self, n, rank, world, shuffle, seed=0):
        self.n, self.rank, self.world, self.shuffle, self.seed, self.epoch = n, rank, world, shuffle, seed, 0

    def __len__(self):
        return self.n // self.world

    def __iter__(self):
        if self.shuffle:
            g = torch.Generator().manual_seed(self.seed + self.epoch)
            order = torch.randperm(self.n, generator=g).tolist()
        else:
            order = list(range(self.n))
        self.epoch += 1
        order = order[:(self.n // self.world) * self.world]
        return iter(order[self.rank::self.world])


def _policy_msg(audio):
    """The message line of a SpecAugment policy (data.audio.augment as a mapping), none for True / False."""
    if not isinstance(audio.get('augment', False), dict):
        return []
    from src.audio import parse_policy
    p = parse_policy(audio['augment'])
    return ['           | SpecAugment policy on the GPU, training batches only: warp {time_warp}, {freq_masks} x F {freq_width}, '
            '{time_masks} x T {time_width} (p {tr}, count ratio {tc}), {fill} fill'.format(
                tr=p['time_ratio_pm'] / 1000.0, tc=p['time_count_ratio_pm'] / 1000.0, **p)]


def load_dataset(n_jobs, use_gpu, pin_memory, ascending, corpus, audio, text, rank=0, world=1, mode=None):
    from functools import partial
    from src.audio import create_transform
    tokenizer = load_text_encoder(**text)
    feat_dim = audio['feat_dim'] * (audio.get('delta_order', 0) + 1)
    path = corpus.get('path', 'synthetic')
    bs = corpus['batch_size']
    if path in ('synthetic', 'synthetic-wav') or not os.path.isdir(path):
        if path not in ('synthetic', 'synthetic-wav'):
            raise FileNotFoundError("corpus path %s does not exist; use 'synthetic' / 'synthetic-wav' or a directory of waveform "
                                    'shards (see src/data.py)' % path)
        wave = path == 'synthetic-wav'
        n_tr = corpus.get('subset', 2000) // bs
        tr = SyntheticLoader(max(n_tr, 1), bs, feat_dim, tokenizer.vocab_size, seed=1 + 104729 * rank, train=(mode != 'eval'), waveform=wave)   # rank r sees its own utterances
        dv = SyntheticLoader(4, bs, feat_dim, tokenizer.vocab_size, seed=2, train=False, max_frames=1200, waveform=wave)
        if wave:
            tr.audio_transform, _ = create_transform(dict(audio), 'train' if mode != 'eval' else 'eval')
            dv.audio_transform, _ = create_transform(dict(audio), 'eval')
        msg = ['Data spec. | Corpus = synthetic LibriSpeech-shaped %s (no corpus on disk)' % ('waveforms' if wave else 'feature batches'),
               'I/O spec.  | Audio Feature = {}\t| Feature Dim = {}\t| Token Type = {}\t| Vocab Size = {}'.format(
                   audio['feat_type'], feat_dim, tokenizer.token_type, tokenizer.vocab_size)]
        if audio.get('time_aug', False):
            msg.append('           | Waveform augmentation (time_aug) on the GPU, training batches only' if wave else
                       "           | time_aug: True ignored: feature batches carry no waveform to augment (use 'synthetic-wav')")
        if wave and mode != 'eval':
            msg.extend(_policy_msg(audio))
        return tr, dv, feat_dim, tokenizer.vocab_size, tokenizer, msg

    # waveform shards on disk
    bucketing = corpus.get('bucketing', False)
    train_split, dev_split = corpus.get('train_split'), corpus.get('dev_split')
    mode = mode or ('train' if train_split is not None else 'eval')
    bucket_size = bs if (bucketing and not ascending and mode == 'train') else 1
    if mode == 'train':
        tr_set = WaveformShardDataset(path, train_split, tokenizer, bucket_size, ascending, corpus.get('subset'))
        dv_set = WaveformShardDataset(path, dev_split, tokenizer, 1)
        tr_bs = 1 if bucketing and not ascending else bs
    else:                            # testing: tr_set = development set, dv_set = test set (reference src/data.py:60-75)
        tr_set = WaveformShardDataset(path, dev_split, tokenizer, 1)
        dv_set = WaveformShardDataset(path, corpus.get('test_split') or dev_split, tokenizer, 1)
        tr_bs = bs
    shuffle = (mode == 'train' and not ascending)
    sampler = _RankShard(len(tr_set), rank, world, shuffle)
    tr = DataLoader(tr_set, batch_size=tr_bs, sampler=sampler, drop_last=shuffle, collate_fn=partial(collect_wav_batch, mode=mode),
                    num_workers=n_jobs, pin_memory=pin_memory)
    dv = DataLoader(dv_set, batch_size=bs, shuffle=False, drop_last=False, collate_fn=partial(collect_wav_batch, mode='eval'),
                    num_workers=n_jobs, pin_memory=pin_memory)
    tr.audio_transform, _ = create_transform(dict(audio), mode)
    dv.audio_transform, _ = create_transform(dict(audio), 'eval')
    msg = ['Data spec. | Corpus = {} (waveform shards from {})'.format(corpus.get('name', '?'), path),
           '           | Train sets = {}\t| Number of utts = {}'.format(train_split, len(tr_set)),
           '           | Dev sets = {}\t| Number of utts = {}'.format(dev_split, len(dv_set)),
           '           | Batch size = {}\t\t| Bucketing = {}'.format(bs, bucketing),
           'I/O spec.  | Audio Feature = {} (GPU front-end)\t| Feature Dim = {}\t| Token Type = {}\t| Vocab Size = {}'.format(
               audio['feat_type'], feat_dim, tokenizer.token_type, tokenizer.vocab_size)]
    if audio.get('time_aug', False) and mode == 'train':
        msg.append('           | Waveform augmentation (time_aug) on the GPU, training batches only')
    if mode == 'train':
        msg.extend(_policy_msg(audio))
    return tr, dv, feat_dim, tokenizer.vocab_size, tokenizer, msg


# ---- text corpora for the RNN language model (reference src/data.py:79-101,182-199, src/collect_batch.py:79-94,
#      corpus/preprocess_librispeech.py:95-151) ---------------------------------------------------------------------------
HALF_BATCHSIZE_TEXT_LEN = 150


class TextDataset(Dataset):
    """Sentences sorted by token count, longest first; with bucketing `__getitem__(i)` returns the bucket of `bucket_size`
    neighbours starting at min(len - bucket, i) (the reference's LibriTextDataset).  Sources per split: `<path>/<split>` as a
    plain text file (one sentence per line, the LibriSpeech LM corpus) or `<path>/<split>/manifest.tsv` of the waveform
    shards (the transcripts)."""

    def __init__(self, path, split, tokenizer, bucket_size):
        self.bucket_size = bucket_size
        sents = []
        for s_ in split:
            f = os.path.join(path, s_)
            man = os.path.join(f, 'manifest.tsv')
            if os.path.isfile(f):
                with open(f, 'r', encoding='utf-8') as fh:
                    sents += [ln.strip() for ln in fh if ln.strip()]
            elif os.path.isfile(man):
                with open(man, 'r', encoding='utf-8') as fh:
                    for ln in fh:
                        cols = ln.rstrip('\n').split('\t')
                        if len(cols) >= 4:
                            sents.append(cols[3])
        assert len(sents) > 0, 'No data found @ {}'.format(path)
        self.text = sorted((tokenizer.encode(t) for t in sents), key=len, reverse=True)

    def __getitem__(self, index):
        if self.bucket_size > 1:
            index = max(0, min(len(self.text) - self.bucket_size, index))
            return self.text[index:index + self.bucket_size]
        return self.text[index]

    def __len__(self):
        return len(self.text)


class SyntheticTextDataset(TextDataset):
    """Random "sentences" over the tokenizer's vocabulary with a first-order structure (token t+1 depends on token t), so a
    language model has something to learn; for plumbing tests and the LM bench (no corpus offline)."""

    def __init__(self, n, vocab_size, bucket_size, seed, max_len=120):
        self.bucket_size = bucket_size
        g = np.random.Generator(np.random.PCG64(seed))
        perm = np.random.Generator(np.random.PCG64(4242)).permutation(vocab_size - 2) + 2      # the same "grammar" for every split
        text = []
        for _ in range(n):
            ln = int(g.integers(8, max_len))
            t = [int(g.integers(2, vocab_size))]
            for _ in range(ln - 1):
                t.append(int(perm[t[-1] - 2]) if g.random() < 0.8 else int(g.integers(2, vocab_size)))
            text.append(t + [1])
        self.text = sorted(text, key=len, reverse=True)


def collect_text_batch(batch, mode):
    """list of token lists or [bucket] -> (B,L) int64, 0-padded; a training batch whose longest sentence exceeds 150 tokens is
    halved (src/collect_batch.py:79-94)."""
    if type(batch[0][0]) is list:
        batch = batch[0]
    if len(batch[0]) > HALF_BATCHSIZE_TEXT_LEN and mode == 'train':
        batch = batch[:len(batch) // 2]
    return torch.nn.utils.rnn.pad_sequence([torch.LongTensor(b) for b in batch], batch_first=True)


def load_textset(n_jobs, use_gpu, pin_memory, corpus, text):
    from functools import partial
    tokenizer = load_text_encoder(**text)
    bs, bucketing = corpus['batch_size'], corpus.get('bucketing', False)
    bucket_size = bs if bucketing else 1
    tr_bs = 1 if bucketing else bs
    path = corpus.get('path', 'synthetic')
    if path == 'synthetic':
        tr_set = SyntheticTextDataset(corpus.get('subset', 4096), tokenizer.vocab_size, bucket_size, seed=11)
        dv_set = SyntheticTextDataset(256, tokenizer.vocab_size, 1, seed=12)
        name = 'synthetic first-order text (no corpus on disk)'
    else:
        if not os.path.isdir(path):
            raise FileNotFoundError("corpus path %s does not exist; use 'synthetic' or a directory (see src/data.py)" % path)
        tr_set = TextDataset(path, corpus['train_split'], tokenizer, bucket_size)
        dv_set = TextDataset(path, corpus['dev_split'], tokenizer, 1)
        name = '{} (from {})'.format(corpus.get('name', '?'), path)
    tr = DataLoader(tr_set, batch_size=tr_bs, shuffle=True, drop_last=True, collate_fn=partial(collect_text_batch, mode='train'),
                    num_workers=0, pin_memory=use_gpu)
    dv = DataLoader(dv_set, batch_size=bs, shuffle=False, drop_last=False, collate_fn=partial(collect_text_batch, mode='eval'),
                    num_workers=0, pin_memory=pin_memory)
    msg = ['Data spec. | Corpus = {}'.format(name),
           '           | Train sets = {}\t| Number of utts = {}'.format(corpus.get('train_split'), len(tr_set)),
           '           | Dev sets = {}\t| Number of utts = {}'.format(corpus.get('dev_split'), len(dv_set)),
           '           | Batch size = {}\t\t| Bucketing = {}'.format(bs, bucketing),
           'I/O spec.  | Token type = {}\t| Vocab size = {}'.format(tokenizer.token_type, tokenizer.vocab_size)]
    return tr, dv, tokenizer.vocab_size, tokenizer, msg
