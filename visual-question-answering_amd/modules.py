"""Callers and feeders of the co-attention path, on stock PyTorch-ROCm.

Everything here is ordinary ``torch.nn`` (MIOpen convolutions / LSTM, hipBLASLt GEMMs): the
image and question encoders stay stock by design (BASELINE.json north_star); only
``co_attention`` is the hand-written HIP path.  Class names, constructor arguments, submodule
attribute names (= ``state_dict`` keys) and ``forward`` signatures follow the reference so that
its checkpoints load and its training loop drives these modules unchanged:

  HierarchicalCoAttentionNet   model.py:157-187      VQABaselineNet            model.py:10-38
  ImageCoAttentionEncoder      model.py:190-243      ImageBaselineEncoder      model.py:41-105
  QuestionCoAttentionEncoder   model.py:246-298      QuestionBaselineEncoder   model.py:108-151
  PhraseConvPool               model.py:301-334      MLPClassifier             model.py:400-434

(PhraseConvPool and MLPClassifier keep the reference's submodules and keys but compute through the HIP library on
CUDA tensors: phrase.py, head.py.)

torchvision is not installed here, so the VGG11-bn topology (cfg "A" + BatchNorm) is spelled
out; a torchvision ``vgg11_bn`` state_dict file loads into it through ``weights_path``.
"""
from __future__ import annotations

import os
from collections import OrderedDict

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

from . import encoder
from .alternating import AlternatingCoAttention
from .coattention import ParallelCoAttention
from .dropout import DropoutState, check_p, feature_dropout
from .head import answer_head

_VGG11_CFG = (64, "M", 128, "M", 256, 256, "M", 512, 512, "M", 512, 512, "M")


def vgg11_bn_features() -> nn.Sequential:
    """conv3x3-BN-ReLU stacks with five 2x2 max-pools: 448x448 -> 14x14x512, 224x224 -> 7x7x512."""
    mods, c_in = [], 3
    for item in _VGG11_CFG:
        if item == "M":
            mods.append(nn.MaxPool2d(2, 2))
            continue
        mods.extend((nn.Conv2d(c_in, item, 3, padding=1), nn.BatchNorm2d(item), nn.ReLU(inplace=True)))
        c_in = item
    return nn.Sequential(*mods)


def _vgg11_bn_classifier_head() -> list:
    """torchvision's classifier minus the final FC-1000 (model.py:93)."""
    return [nn.Linear(512 * 7 * 7, 4096), nn.ReLU(True), nn.Dropout(), nn.Linear(4096, 4096), nn.ReLU(True),
            nn.Dropout()]


def _load_vgg_weights(features: nn.Module, classifier: nn.Module | None, weights_path):
    """Load a torchvision vgg11_bn state_dict file if one is given and present (model.py:232-233).
    Without a file the reference would download pretrained weights; there is no network here, so
    the encoder keeps its random init."""
    if not weights_path or not os.path.isfile(str(weights_path)):
        return False
    sd = torch.load(weights_path, map_location="cpu")
    features.load_state_dict({k[len("features."):]: v for k, v in sd.items() if k.startswith("features.")})
    if classifier is not None:
        cls = {k[len("classifier."):]: v for k, v in sd.items() if k.startswith("classifier.")}
        classifier.load_state_dict({k: v for k, v in cls.items() if not k.startswith("6.")}, strict=False)
    return True


def run_conv_bn_stack(seq: nn.Sequential, x: torch.Tensor, eval_impl: str = "stock") -> torch.Tensor:
    """Runs a Conv2d / BatchNorm2d / ReLU / MaxPool2d ``Sequential`` (the VGG ``features``) with the
    same stock kernels but two value-preserving graph rewrites that save whole elementwise passes
    over the largest activations:

    * ``MaxPool2d(ReLU(x)) == ReLU(MaxPool2d(x))`` exactly (both are monotonic): the ReLU runs on the
      4x smaller pooled tensor.
    * A frozen Conv2d bias in front of a BatchNorm2d that normalises with BATCH statistics (train
      mode -- the reference never calls ``.eval()`` on its frozen VGG, model.py:239-241) cancels in
      ``(y + b) - mean(y + b)``: the convolution is issued without bias (saves the separate
      broadcast-add kernel) and ``momentum * b`` is added to ``running_mean`` instead, which is the
      only place the bias survives (running_var is shift-invariant).  Outputs differ from the plain
      graph by fp32 rounding only (tests/test_net_cpu.py).

    On top of them, where the tensor is CUDA fp32 channels_last and autograd need not record the step (a frozen encoder, or
    no_grad), the HIP library takes over memory-bound glue (``encoder.py``, csrc/encoder.hip); the convolutions stay on MIOpen:

    * by default ``ReLU(MaxPool2d(2, 2)(x))`` runs as ONE pass (``encoder.relu_pool``) instead of two kernels; both operations are
      exact, so every value keeps its bits;
    * by default too, a whole ``Conv2d -> BatchNorm2d -> ReLU [-> MaxPool2d(2, 2)]`` group runs everything after the convolution
      in two passes that sum in MIOpen's order with MIOpen's formula (``encoder.bn_exact``): the stock chain's bits.  Only for a
      shape whose first call in this process, which runs the stock chain, found the two equal in every bit
      (``encoder.bn_exact_or_stock``, ``encoder.exact_report()``); ``VQA_ENCODER_EXACT_BN=0`` turns it off.  The frozen
      convolution bias stays the separate ``running_mean.add_`` it is on the stock route;
    * by default too, the FIRST group, where it is the VGG's 3 -> 64 channel 3x3 convolution on a channels_last image with
      channels_last weights, runs the convolution itself in the kernel that sums the statistics, in the stock convolution's
      arithmetic (``encoder.conv1_bn_exact_or_stock``): no zero fill, no separate statistics pass.  Verified per shape against the
      stock convolution and chain like the route above, or not used; ``VQA_ENCODER_EXACT_CONV1=0`` turns it off.  The
      convolution is computed twice, once for the statistics and once to be normalised, and its output never stored;
      ``VQA_ENCODER_CONV1_RECOMPUTE=0`` keeps the form that stores it and reads it back;
    * with ``VQA_ENCODER_FUSED=1`` a whole ``Conv2d -> BatchNorm2d -> ReLU [-> MaxPool2d(2, 2)]`` group runs everything after the
      convolution in two passes over its output (``encoder.bn_relu_pool``), the bias fold included.  Its statistics are summed
      in double, in another order than MIOpen's: values agree with the stock chain to rounding, not bit for bit.

    ``VQA_ENCODER_FUSED=0`` keeps the stock kernels.

    EVAL-mode BatchNorm (``Trainer.validate``, ``predict.py``, ``extract.py``) is executed as is by default
    (``eval_impl="stock"``: the convolution with its bias, the stock BatchNorm, then the ReLU / pool pass above).  With
    ``eval_impl="hip"`` a whole ``Conv2d -> BatchNorm2d -> ReLU [-> MaxPool2d(2, 2)]`` group whose BatchNorm normalises with its
    running statistics runs everything after the convolution -- the bias add, the BatchNorm, the ReLU, the pool -- in ONE launch
    in the stock inference kernel's arithmetic (``encoder.bn_eval_or_stock``), and the first group runs in one launch from the
    image (``encoder.conv1_bn_eval_or_stock``).  Per shape verified against the stock chain on its first call like the routes
    above, or not used (``encoder.eval_report()``).  Under ``encoder.eval_group_fusable``'s conditions only -- a CUDA tensor, a
    frozen group or no_grad, no autocast -- and never for a train-mode BatchNorm, whose branches below do not look at ``eval_impl``.

    Anything that does not match these patterns (trainable bias, NCHW, autocast, other modules) is executed as is.
    ``VQA_ENCODER_REWRITE=0`` disables all of it."""
    mods = list(seq)
    if eval_impl not in encoder.EVAL_IMPLS:
        raise ValueError("eval_impl must be one of %s, got %r" % (encoder.EVAL_IMPLS, eval_impl))
    if os.environ.get("VQA_ENCODER_REWRITE", "1") == "0":
        return seq(x)
    i, n = 0, len(mods)
    while i < n:
        m = mods[i]
        nxt = mods[i + 1] if i + 1 < n else None
        pool = mods[i + 3] if i + 3 < n and isinstance(mods[i + 3], nn.MaxPool2d) else None
        group = isinstance(m, nn.Conv2d) and isinstance(nxt, nn.BatchNorm2d) and i + 2 < n and isinstance(mods[i + 2], nn.ReLU)
        if eval_impl == "hip" and group and not nxt.training and encoder.eval_group_fusable(m, nxt, pool, x):
            if i == 0 and encoder.conv1_eval_inputs_fusable(x, m, nxt, pool is not None):
                x = encoder.conv1_bn_eval_or_stock(x, m, nxt, pool)
            else:
                x = encoder.bn_eval_or_stock(x, m, nxt, pool)
            i += 3 if pool is None else 4
            continue
        fuse = group and encoder.modules_fusable(m, nxt, pool, x)
        exact = group and encoder.exact_modules_fusable(m, nxt, pool, x)
        if (isinstance(m, nn.Conv2d) and (fuse or exact or (m.bias is not None and not m.bias.requires_grad))
                and m.padding_mode == "zeros" and isinstance(nxt, nn.BatchNorm2d) and nxt.training and nxt.momentum is not None):
            if exact and i == 0 and encoder.conv1_modules_fusable(m, nxt, pool, x):
                x = encoder.conv1_bn_exact_or_stock(x, m, nxt, pool)
                if m.bias is not None:
                    with torch.no_grad():
                        nxt.running_mean.add_(m.bias.to(nxt.running_mean.dtype), alpha=nxt.momentum)
                i += 3 if pool is None else 4
                continue
            x = F.conv2d(x, m.weight, None, m.stride, m.padding, m.dilation, m.groups)
            if fuse and encoder.output_fusable(x, nxt, pool is not None):
                x = encoder.bn_relu_pool(x, nxt, conv_bias=m.bias, pool=pool is not None)
                i += 3 if pool is None else 4
                continue
            exact = exact and encoder.exact_output_fusable(x, nxt, pool is not None)
            x = encoder.bn_exact_or_stock(x, nxt, pool) if exact else nxt(x)
            if m.bias is not None and nxt.track_running_stats and nxt.running_mean is not None:
                with torch.no_grad():
                    nxt.running_mean.add_(m.bias.to(nxt.running_mean.dtype), alpha=nxt.momentum)
            i += 2 if not exact else 3 if pool is None else 4
        elif isinstance(m, nn.ReLU) and isinstance(nxt, nn.MaxPool2d):
            x = encoder.relu_pool(x) if encoder.relu_pool_fusable(nxt, x) else F.relu(nxt(x), inplace=True)
            i += 2
        else:
            x = m(x)
            i += 1
    return x


class ImageCoAttentionEncoder(nn.Module):
    """VGG11-bn ``features`` -> spatial grid [B, N, 512] (a permuted view of [B, 512, N])."""

    def __init__(self, is_trainable, weights_path):
        super().__init__()
        self.is_trainable = is_trainable
        self.weights_path = weights_path
        self.vgg11_encoder = vgg11_bn_features()
        _load_vgg_weights(self.vgg11_encoder, None, weights_path)
        self.flatten = nn.Flatten(start_dim=2, end_dim=3)
        self.eval_impl = "stock"       # eval-mode groups: "stock" or "hip" (run_conv_bn_stack; a plain attribute, not state)
        if not is_trainable:                      # frozen; BatchNorm stays in train mode (model.py:239-241)
            for prm in self.vgg11_encoder.parameters():
                prm.requires_grad = False

    def forward(self, x_img):
        grid = self.flatten(run_conv_bn_stack(self.vgg11_encoder, x_img, self.eval_impl))      # [B, 512, N]
        return grid.permute(0, 2, 1)                         # [B, N, 512] view, strides (512N, 1, N)


class _Bottleneck(nn.Module):
    """torchvision's ResNet bottleneck (1x1 -> 3x3 (stride) -> 1x1 x4, BatchNorm, residual)."""

    def __init__(self, c_in, width, stride, downsample):
        super().__init__()
        self.conv1 = nn.Conv2d(c_in, width, 1, bias=False); self.bn1 = nn.BatchNorm2d(width)
        self.conv2 = nn.Conv2d(width, width, 3, stride=stride, padding=1, bias=False); self.bn2 = nn.BatchNorm2d(width)
        self.conv3 = nn.Conv2d(width, 4 * width, 1, bias=False); self.bn3 = nn.BatchNorm2d(4 * width)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample

    def forward(self, x):
        idt = x if self.downsample is None else self.downsample(x)
        y = self.relu(self.bn1(self.conv1(x)))
        y = self.relu(self.bn2(self.conv2(y)))
        return self.relu(self.bn3(self.conv3(y)) + idt)


def resnet152_features() -> nn.Sequential:
    """ResNet-152 trunk (stem + layers [3, 8, 36, 3]) up to the 2048-channel stride-32 map:
    224x224 -> 7x7x2048 (BASELINE config 4).  Stock torch.nn; torchvision-compatible topology."""
    mods = [nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False), nn.BatchNorm2d(64), nn.ReLU(inplace=True),
            nn.MaxPool2d(3, stride=2, padding=1)]
    c_in = 64
    for width, blocks, stride in ((64, 3, 1), (128, 8, 2), (256, 36, 2), (512, 3, 2)):
        for i in range(blocks):
            st = stride if i == 0 else 1
            ds = None
            if st != 1 or c_in != 4 * width:
                ds = nn.Sequential(nn.Conv2d(c_in, 4 * width, 1, stride=st, bias=False), nn.BatchNorm2d(4 * width))
            mods.append(_Bottleneck(c_in, width, st, ds))
            c_in = 4 * width
    return nn.Sequential(*mods)


class ImageResNetCoAttentionEncoder(nn.Module):
    """BASELINE config 4 feeder (an extension; the reference only ships the VGG encoder): frozen
    ResNet-152 trunk -> spatial grid [B, N, 2048] as a permuted view of [B, 2048, N]."""

    def __init__(self, is_trainable=False, weights_path=None):
        super().__init__()
        self.is_trainable, self.weights_path = is_trainable, weights_path
        self.resnet_encoder = resnet152_features()
        self.flatten = nn.Flatten(start_dim=2, end_dim=3)
        if not is_trainable:
            for prm in self.resnet_encoder.parameters():
                prm.requires_grad = False

    def forward(self, x_img):
        return self.flatten(self.resnet_encoder(x_img)).permute(0, 2, 1)


class PhraseConvPool(nn.Module):
    """1/2/3-gram Conv1d + tanh, then a max over 3 CONSECUTIVE channels of the concatenated
    [uni|bi|tri] vector -- the reference's reshape (model.py:324-332) groups channels 3e..3e+2,
    not the three n-gram responses of one channel; reproduced as is."""

    def __init__(self, emb_dim):
        super().__init__()
        self.conv_unigram = nn.Sequential(nn.ConstantPad1d((0, 0), 0), nn.Conv1d(emb_dim, emb_dim, 1, 1), nn.Tanh())
        self.conv_bigram = nn.Sequential(nn.ConstantPad1d((1, 0), 0), nn.Conv1d(emb_dim, emb_dim, 2, 1), nn.Tanh())
        self.conv_trigram = nn.Sequential(nn.ConstantPad1d((1, 1), 0), nn.Conv1d(emb_dim, emb_dim, 3, 1), nn.Tanh())
        self.max_pool = nn.MaxPool2d(kernel_size=(1, 3))
        self.fast_products = False     # tolerance mode of the HIP path's fp32 products (train.Trainer(precision="fast") sets it)

    def forward(self, x_question):
        if x_question.is_cuda and os.environ.get("VQA_PHRASE_IMPL", "hip") != "stock":
            # MI355X path (csrc/phrase.hip): same parameters, same values; stock modules below on CPU
            from .phrase import phrase_conv_pool
            u, b, t = self.conv_unigram[1], self.conv_bigram[1], self.conv_trigram[1]
            return phrase_conv_pool(x_question, u.weight, u.bias, b.weight, b.bias, t.weight, t.bias,
                                    fast=self.fast_products)
        B, T, E = x_question.shape
        x = x_question.permute(0, 2, 1)                                          # [B, E, T]
        grams = torch.cat([self.conv_unigram(x), self.conv_bigram(x), self.conv_trigram(x)], dim=1)
        grams = grams.permute(0, 2, 1).reshape(B, T, E, 3)                       # groups of 3 consecutive channels
        return self.max_pool(grams).squeeze(dim=3)                               # [B, T, E]


SENTENCE_IMPLS = ("stock", "hip")


def _hip_sentence(enc, phrases) -> bool:
    """Does this forward of a question encoder take the HIP sentence LSTM on `phrases`, the LSTM's input?
    ``enc.sentence_impl``: "stock" (the default: pack_padded_sequence -> nn.LSTM -> pad_packed_sequence) or "hip"
    (lstm.sentence_lstm on the nn.LSTM's own parameters: a CUDA input of a supported shape that is fp32, or any floating
    type under CUDA autocast, where sentence_lstm is an fp32 island that casts it -- the BERT encoder's bf16 word level;
    CPU tensors, other shapes and other dtypes outside autocast take the stock lines)."""
    impl = enc.sentence_impl
    if impl not in SENTENCE_IMPLS:
        raise ValueError("sentence_impl must be one of %s, got %r" % (SENTENCE_IMPLS, impl))
    if impl != "hip" or not phrases.is_cuda:
        return False
    if phrases.dtype != torch.float32 and not (phrases.is_floating_point() and torch.is_autocast_enabled("cuda")):
        return False
    from . import lstm
    B, T, E = phrases.shape
    return lstm.supported(B, T, E, enc.sentence_lstm.hidden_size)


def _hip_sentence_lstm(rnn, phrases, x_lens):
    from .lstm import sentence_lstm
    return sentence_lstm(phrases, x_lens, rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0, rnn.bias_hh_l0)


WORD_IMPLS = ("stock", "hip")


def _hip_words(enc, x) -> bool:
    """Does this forward of the question encoder take the HIP word embedding on the ids `x`?  ``enc.word_impl``: "stock"
    (the default: nn.Embedding's forward) or "hip" (embedding.word_embedding on the nn.Embedding's own weight and
    padding_idx: ids on CUDA, an fp32 weight, a supported shape; CPU tensors, other dtypes and shapes take the stock line)."""
    impl = enc.word_impl
    if impl not in WORD_IMPLS:
        raise ValueError("word_impl must be one of %s, got %r" % (WORD_IMPLS, impl))
    emb = enc.word_embedding
    if impl != "hip" or not x.is_cuda or not emb.weight.is_cuda or emb.weight.dtype != torch.float32:
        return False
    if x.is_floating_point() or emb.max_norm is not None or emb.scale_grad_by_freq or emb.sparse:
        return False
    from . import embedding
    return embedding.supported(x.numel(), emb.num_embeddings, emb.embedding_dim)


class QuestionCoAttentionEncoder(nn.Module):
    """word (embedding) / phrase (n-gram conv + pool) / sentence (LSTM) features, each [B,T,hidden];
    rows past a question's length are exact zeros at all three levels (padding_idx=0, packed LSTM).
    ``sentence_impl``: "stock" (default) or "hip" (`_hip_sentence`); ``word_impl``: "stock" (default) or "hip"
    (`_hip_words`); parameters and state_dict are the same either way."""

    def __init__(self, vocab_size, word_emb_dim, hidden_dim):
        super().__init__()
        self.vocab_size, self.embedding_dim, self.hidden_dim = vocab_size, word_emb_dim, hidden_dim
        self.word_embedding = nn.Embedding(vocab_size, word_emb_dim, padding_idx=0)
        self.phrase_conv_pool = PhraseConvPool(word_emb_dim)
        self.sentence_lstm = nn.LSTM(word_emb_dim, hidden_dim)
        self.sentence_impl = "stock"
        self.word_impl = "stock"

    def forward(self, x, x_lens):
        T = x.shape[1]
        if _hip_words(self, x):                                       # opt-in: csrc/embedding.hip, ids stay on the device
            from .embedding import word_embedding
            words = word_embedding(x, self.word_embedding.weight, self.word_embedding.padding_idx)
        else:
            words = self.word_embedding(x)
        phrases = self.phrase_conv_pool(words)
        if _hip_sentence(self, phrases):                              # opt-in: csrc/lstm.hip, lengths stay on the device
            sentence, phrases = _hip_sentence_lstm(self.sentence_lstm, phrases, x_lens)
            return words, phrases, sentence
        lens = x_lens.cpu() if torch.is_tensor(x_lens) else x_lens    # pack_padded_sequence wants CPU lengths
        phrases = pack_padded_sequence(phrases, lens, batch_first=True)
        sentence, _ = self.sentence_lstm(phrases)
        phrases = pad_packed_sequence(phrases, batch_first=True, total_length=T)[0]
        sentence = pad_packed_sequence(sentence, batch_first=True, total_length=T)[0]
        return words, phrases, sentence


class QuestionBertCoAttentionEncoder(nn.Module):
    """BASELINE config 5 (an extension: the reference lists BERT as a TODO, README.md:137-141, and its
    ``--model bert`` flag has no registry entry): the word level of the hierarchy comes from frozen
    768-d token embeddings of a BERT-base encoder, projected to ``hidden_dim``; phrase and sentence
    levels are built on top of it exactly as in QuestionCoAttentionEncoder.  ``bert`` is any module
    mapping token ids [B,T] to [B,T,bert_dim] (e.g. ``transformers.BertModel(...).embeddings``); it is
    frozen.  Pad rows are re-zeroed so that the three levels keep the reference's zero-pad invariant."""

    def __init__(self, bert: nn.Module, bert_dim, hidden_dim):
        super().__init__()
        self.bert = bert
        for prm in self.bert.parameters():
            prm.requires_grad = False
        self.word_proj = nn.Linear(bert_dim, hidden_dim)
        self.phrase_conv_pool = PhraseConvPool(hidden_dim)
        self.sentence_lstm = nn.LSTM(hidden_dim, hidden_dim)
        self.sentence_impl = "stock"                    # as QuestionCoAttentionEncoder.sentence_impl
        self.hidden_dim = hidden_dim
        self.bert.eval()

    def train(self, mode: bool = True):
        """The frozen token-embedding module stays in eval mode (its dropout would make the "frozen embeddings"
        of BASELINE config 5 random)."""
        super().train(mode)
        self.bert.eval()
        return self

    def forward(self, x, x_lens):
        T = x.shape[1]
        with torch.no_grad():
            tok = self.bert(x)
            tok = tok[0] if isinstance(tok, (tuple, list)) else getattr(tok, "last_hidden_state", tok)
        words = self.word_proj(tok) * (x != 0).unsqueeze(-1).to(tok.dtype)     # zero the pad rows
        phrases = self.phrase_conv_pool(words)
        if _hip_sentence(self, phrases):                              # (decided on the LSTM's input, fp32 under autocast too)
            sentence, phrases = _hip_sentence_lstm(self.sentence_lstm, phrases, x_lens)
            return words, phrases, sentence
        lens = x_lens.cpu() if torch.is_tensor(x_lens) else x_lens
        phrases = pack_padded_sequence(phrases, lens, batch_first=True)
        sentence, _ = self.sentence_lstm(phrases)
        phrases = pad_packed_sequence(phrases, batch_first=True, total_length=T)[0]
        sentence = pad_packed_sequence(sentence, batch_first=True, total_length=T)[0]
        return words, phrases, sentence


class MLPClassifier(nn.Module):
    """Recursive word -> phrase -> sentence answer head (model.py:400-434): same constructor, submodules and
    state_dict keys as the reference class.  CUDA fp32 tensors take the HIP head (``head.answer_head``: adds,
    concatenations, bias + tanh folded into tile products on the exact-fp32 MFMA); CPU tensors, or
    ``VQA_HEAD_IMPL=stock``, the stock ``nn.Linear`` modules."""

    def __init__(self, hidden_dim, mlp_dim, K):
        super().__init__()
        self.W_w = nn.Linear(hidden_dim, hidden_dim)
        self.W_p = nn.Linear(2 * hidden_dim, hidden_dim)
        self.W_s = nn.Linear(2 * hidden_dim, mlp_dim)
        self.W_h = nn.Linear(mlp_dim, K)
        self.bf16_products = False       # reduced-precision mode of the HIP head (set with --opt_lvl >= 1, train.Trainer)

    def _hip(self, x):
        x0 = x if torch.is_tensor(x) else x[0]
        return x0.is_cuda and os.environ.get("VQA_HEAD_IMPL", "hip") != "stock"

    def _params(self):
        return (self.W_w.weight, self.W_w.bias, self.W_p.weight, self.W_p.bias, self.W_s.weight, self.W_s.bias,
                self.W_h.weight, self.W_h.bias)

    def forward(self, x_img_feats, x_ques_feats):
        if self._hip(x_img_feats):
            return answer_head(x_img_feats, x_ques_feats, *self._params(), bf16=self.bf16_products)
        (q_w, q_p, q_s), (v_w, v_p, v_s) = x_ques_feats, x_img_feats
        h_w = torch.tanh(self.W_w(q_w + v_w))
        h_p = torch.tanh(self.W_p(torch.cat([q_p + v_p, h_w], dim=1)))
        h_s = torch.tanh(self.W_s(torch.cat([q_s + v_s, h_p], dim=1)))
        return self.W_h(h_s)

    def forward_loss(self, x_img_feats, x_ques_feats, labels=None, targets=None, loss_kind="soft_ce"):
        """(logits, nn.CrossEntropyLoss()(logits, labels)) -- main.py:211 + :214 -- in one call of the HIP head.
        targets = (ans_idx int32 [B,A], ans_score fp32 [B,A]) instead of labels: (logits, the soft-target loss `loss_kind`
        of loss.soft_target_loss) -- VQA's ten human answers instead of the majority answer."""
        if (labels is None) == (targets is None):
            raise ValueError("forward_loss: give labels or targets (one of the two)")
        if self._hip(x_img_feats):
            if targets is not None:
                return answer_head(x_img_feats, x_ques_feats, *self._params(), bf16=self.bf16_products, targets=targets,
                                   loss_kind=loss_kind)
            return answer_head(x_img_feats, x_ques_feats, *self._params(), labels=labels, bf16=self.bf16_products)
        logits = self.forward(x_img_feats, x_ques_feats)
        if targets is not None:
            from .loss import soft_target_loss_stock
            return logits, soft_target_loss_stock(logits.float(), targets[0], targets[1], loss_kind)
        return logits, F.cross_entropy(logits.float(), labels)


class HierarchicalCoAttentionNet(nn.Module):
    """question encoder -> image encoder -> co-attention (HIP) -> MLP logits [B, K].
    co_attention: "parallel" (the default: ParallelCoAttention, the reference's form) or "alternating"
    (AlternatingCoAttention, Lu et al. 2016 section 3.3; it always takes the per-module path, never the hot-path node)."""

    CO_ATTENTIONS = ("parallel", "alternating")

    def __init__(self, ques_enc_params, img_enc_params, K, mlp_dim=1024, co_attention="parallel"):
        super().__init__()
        self.hidden_dim = ques_enc_params["hidden_dim"]
        img_enc_params = dict(img_enc_params)
        if img_enc_params.pop("arch", "vgg11_bn") == "resnet152":     # config 4 extension (2048-channel grid)
            self.image_encoder = ImageResNetCoAttentionEncoder(**img_enc_params)
        else:
            self.image_encoder = ImageCoAttentionEncoder(**img_enc_params)
        if "bert" in ques_enc_params:                 # config 5 extension; the reference has only the LSTM path
            self.question_encoder = QuestionBertCoAttentionEncoder(**ques_enc_params)
        else:
            self.question_encoder = QuestionCoAttentionEncoder(**ques_enc_params)
        if co_attention not in self.CO_ATTENTIONS:
            raise ValueError("co_attention must be one of %s, got %r" % (self.CO_ATTENTIONS, co_attention))
        self.co_attention_form = co_attention
        self.co_attention = (AlternatingCoAttention(self.hidden_dim) if co_attention == "alternating"
                             else ParallelCoAttention(self.hidden_dim))
        self.mlp_classify = MLPClassifier(self.hidden_dim, mlp_dim, K)
        self.hot_path_graph = False                   # opt-in: replay the hot path from a captured HIP graph (graph.py)
        # train.Trainer's default on CUDA: the hot path as ONE autograd node over static buffers, its C-ABI calls issued
        # eagerly (graph.HotPathGraph(capture=False)); hot_path_direct_grads: the static gradient buffers become param.grad
        self.hot_path_static = False
        self.hot_path_direct_grads = False
        self._graphs = {}
        # feature dropout (dropout.py; set_feature_dropout): probability applied in training to the six attended features in
        # front of the answer head, and the device-side state its masks are drawn from.  Neither is part of the state_dict.
        self.feature_dropout = 0.0
        self.dropout_state = None

    def forward(self, x_img, x_ques, x_ques_lens, return_attention=False, targets=None, loss_kind="soft_ce"):
        return self.forward_features(self.image_encoder(x_img), x_ques, x_ques_lens, return_attention=return_attention,
                                     targets=targets, loss_kind=loss_kind)

    def forward_features(self, x_img_features, x_ques, x_ques_lens, labels=None, return_attention=False, targets=None,
                         loss_kind="soft_ce"):
        """The forward pass from already-encoded image features [B,N,d] (model.py:171-187 minus the
        image encoder call): lets a frozen encoder run ahead on its own stream (train.Trainer).
        `x_img_features` may be a zero-argument callable returning the features.  With `labels` (int64 [B]) the
        mean cross entropy of main.py:214 comes out of the answer head's own call: returns (logits, loss).
        `x_ques_lens` reaches the co-attention too when its ``question_mask`` is on (ParallelCoAttention).
        return_attention=True: the co-attention maps a_v [3,B,N], a_q [3,B,T] come out as well -- (logits, a_v, a_q), or
        (logits, loss, a_v, a_q) with `labels` -- differentiable, for a loss on them (ParallelCoAttention.forward).  This
        takes the per-module path, never the hot-path node (`hot_path_static` / `hot_path_graph`).
        targets = (ans_idx int32 [B,A], ans_score fp32 [B,A]) in place of `labels`: the loss is the soft-target loss
        `loss_kind` ("soft_ce" | "bce", loss.soft_target_loss); everything above holds with "labels" read as "targets".
        In training mode with ``feature_dropout`` > 0 (set_feature_dropout) every route -- per-module, with the attention
        maps, the alternating form, the hot-path node -- drops the six attended features in front of the answer head under one
        mask drawn from ``dropout_state`` (dropout.py); in eval mode, or with 0, none does and the state is not touched."""
        if labels is not None and targets is not None:
            raise ValueError("forward_features: give labels or targets, not both")
        if targets is not None and loss_kind not in ("soft_ce", "bce"):
            raise ValueError("loss_kind must be 'soft_ce' or 'bce', got %r" % (loss_kind,))
        has_loss = labels is not None or targets is not None
        tk = dict(targets=targets, loss_kind=loss_kind) if targets is not None else dict(labels=labels)
        x_ques_features = list(self.question_encoder(x_ques, x_ques_lens))
        if callable(x_img_features):            # resolved only now: the question side is queued first
            x_img_features = x_img_features()
        masked = self._question_mask()
        drop = self._dropout_p()
        if return_attention:
            lens = (x_ques_lens,) if masked else ()
            v, q, a_v, a_q = self.co_attention(x_img_features, x_ques_features, *lens, return_attention=True)
            if drop:
                v, q = feature_dropout(v, q, drop, self.dropout_state)
            if has_loss:
                return (*self.mlp_classify.forward_loss(v, q, **tk), a_v, a_q)
            return self.mlp_classify(v, q), a_v, a_q
        if (has_loss and (self.hot_path_graph or self.hot_path_static) and x_img_features.is_cuda
                and torch.is_grad_enabled() and self.co_attention_form == "parallel"):     # (the node is parallel-only)
            return self._graphed(x_img_features, x_ques_features, labels, x_ques_lens if masked else None, targets=targets,
                                 loss_kind=loss_kind, dropout=drop)
        if masked:
            x_img_attn, x_ques_attn = self.co_attention(x_img_features, x_ques_features, x_ques_lens)
        else:
            x_img_attn, x_ques_attn = self.co_attention(x_img_features, x_ques_features)
        if drop:
            x_img_attn, x_ques_attn = feature_dropout(x_img_attn, x_ques_attn, drop, self.dropout_state)
        if has_loss:
            return self.mlp_classify.forward_loss(x_img_attn, x_ques_attn, **tk)
        return self.mlp_classify(x_img_attn, x_ques_attn)

    def forward_with_attention(self, x_img, x_ques, x_ques_lens):
        """Inference with the co-attention maps: (logits [B,K], a_v [3,B,N], a_q [3,B,T]) for the word, phrase and sentence
        levels.  Index n of a_v is location n of the encoder's flattened grid (model.py:215-217: row-major over 7 x 7 at
        224 px, 14 x 14 at 448 px); a_q is unmasked over the T token positions (model.py:388) -- or, with the co-attention's
        ``question_mask`` on, 0 past each question's length.  The logits equal `forward`'s under no_grad bit for bit -- in eval
        mode or with ``feature_dropout = 0``: this is the inference call and never applies dropout, `forward` does in training.
        Forward only: raises where a gradient would be needed."""
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise RuntimeError("forward_with_attention is forward only: run it under torch.no_grad()")
        return self.forward_features_with_attention(self.image_encoder(x_img), x_ques, x_ques_lens)

    def forward_features_with_attention(self, x_img_features, x_ques, x_ques_lens):
        """`forward_with_attention` from already-encoded image features [B,N,d] (the rows of a feature table,
        features.gather_features): the image encoder is not called.  Same results, same restrictions."""
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise RuntimeError("forward_features_with_attention is forward only: run it under torch.no_grad()")
        x_ques_features = [q if q.dtype == torch.float32 else q.float()       # (the fp32 island, as _CoAttentionFn's cast)
                           for q in self.question_encoder(x_ques, x_ques_lens)]
        if self._question_mask():
            v, q, a_v, a_q = self.co_attention.forward_with_attention(x_img_features, x_ques_features, x_ques_lens)
        else:
            v, q, a_v, a_q = self.co_attention.forward_with_attention(x_img_features, x_ques_features)
        return self.mlp_classify(v, q), a_v, a_q

    def _question_mask(self) -> bool:
        return bool(getattr(self.co_attention, "question_mask", False))

    def _dropout_p(self) -> float:
        """The feature-dropout probability of this forward: 0 in eval mode (the state is then never touched)."""
        p = float(self.feature_dropout) if self.training else 0.0
        if p and self.dropout_state is None:
            raise RuntimeError("feature_dropout = %g without a dropout_state: use set_feature_dropout(model, p, seed)" % p)
        return p

    def _graphed(self, x_img_features, x_ques_features, labels, x_ques_lens=None, targets=None, loss_kind="soft_ce",
                 dropout=0.0):
        """co-attention + answer head + loss, forward AND backward, as one autograd node over static buffers (graph.py),
        built per (B, N, T) on first use: replayed from captured HIP graphs (``net.hot_path_graph = True``,
        ``Trainer(graph=True)``) or with its four C-ABI calls issued eagerly (``net.hot_path_static``, the Trainer's
        default)."""
        from . import _lib
        from .graph import HotPathGraph
        if self.co_attention_form != "parallel":
            raise RuntimeError("the hot-path node (graph.HotPathGraph) serves the parallel co-attention only")
        B, N, _ = x_img_features.shape
        T = x_ques_features[0].shape[1]
        key = (B, N, T, bool(x_img_features.requires_grad), bool(self.co_attention.bf16_projections),
               bool(self.mlp_classify.bf16_products), bool(self.hot_path_graph), bool(self.hot_path_direct_grads),
               bool(self.co_attention.fast_products), self._question_mask(),
               ("ce", 0) if targets is None else (loss_kind, int(targets[0].shape[1])),
               (dropout, self.dropout_state.data_ptr()) if dropout else (0.0, 0),   # p and the state's address
               getattr(self.co_attention, "affinity", "reference"))
        hp = self._graphs.get(key)
        # (the node reads the parameters where they lie: one built before the module was moved -- .to(), .cuda(), new
        #  Parameter objects -- would read the old storage)
        if hp is not None and hp.stale():          # (all 16 parameters: any of them may have been replaced or re-pointed -- ADVICE r4)
            hp = None
        if hp is None:
            hp = self._graphs[key] = HotPathGraph(self.co_attention, self.mlp_classify, B, N, T, need_dv=key[3],
                                                  flags=(_lib.FLAG_BF16_PROJ if key[4] else 0) | _lib.precision_flag(key[8] and not key[4]),
                                                  capture=key[6], direct_grads=key[7], question_mask=key[9],
                                                  **({} if targets is None else dict(loss=key[10][0], num_answers=key[10][1])),
                                                  **(dict(dropout=dropout, dropout_state=self.dropout_state) if dropout else {}))
        return hp(x_img_features, x_ques_features, labels if targets is None else targets, q_len=x_ques_lens)


# ---- baseline model (BASELINE config 1: stock PyTorch plumbing by default; on request the question GRU on csrc/gru.hip and
# everything behind the two encoders -- row norm, the two embeddings, the product, Linear -> Dropout -> Tanh with the dropout
# drawn inside the head, the classifier -- on csrc/fusion.hip) -------------------------------------------------------------
class ImageBaselineEncoder(nn.Module):
    """VGG11-bn up to fc7 (4096), L2-normalised, -> 1024 tanh."""

    def __init__(self, is_trainable, weights_path):
        super().__init__()
        self.is_trainable, self.weights_path = is_trainable, weights_path
        features = vgg11_bn_features()
        head = nn.Sequential(*_vgg11_bn_classifier_head())
        _load_vgg_weights(features, head, weights_path)
        self.vgg11_encoder = nn.Sequential(OrderedDict([
            ("conv_layers", features), ("avgpool", nn.AdaptiveAvgPool2d((7, 7))),
            ("fc_layers", nn.Sequential(nn.Flatten(), *list(head)))]))
        self.embedding_layer = nn.Sequential(nn.Linear(4096, 1024), nn.Tanh())
        if not is_trainable:
            for prm in self.vgg11_encoder.parameters():
                prm.requires_grad = False

    def forward(self, x_img):
        return self.embedding_layer(F.normalize(self.vgg11_encoder(x_img), dim=1, p=2))


GRU_IMPLS = ("stock", "hip")


def _hip_gru(enc, emb) -> bool:
    """Does this forward of the baseline's question encoder take the HIP GRU on `emb`, the GRU's input?  ``enc.gru_impl``:
    "stock" (the default: pack_padded_sequence -> nn.GRU) or "hip" (gru.question_gru on the nn.GRU's own parameters: a CUDA
    input of a supported shape that is fp32, or any floating type under CUDA autocast, where question_gru is an fp32 island
    that casts it, and an nn.GRU of one layer, one direction, with bias and without dropout; CPU tensors, other shapes,
    other dtypes outside autocast and other GRUs take the stock lines)."""
    impl = enc.gru_impl
    if impl not in GRU_IMPLS:
        raise ValueError("gru_impl must be one of %s, got %r" % (GRU_IMPLS, impl))
    if impl != "hip" or not emb.is_cuda:
        return False
    if emb.dtype != torch.float32 and not (emb.is_floating_point() and torch.is_autocast_enabled("cuda")):
        return False
    rnn = enc.gru
    if not isinstance(rnn, nn.GRU) or rnn.num_layers != 1 or rnn.bidirectional or not rnn.bias or rnn.dropout != 0:
        return False
    from . import gru
    B, T, E = emb.shape
    return E == rnn.input_size and gru.supported(B, T, E, rnn.hidden_size)


class QuestionBaselineEncoder(nn.Module):
    """Embedding + tanh -> GRU (last non-pad state via packing) -> 1024 tanh.
    ``gru_impl``: "stock" (default) or "hip" (`_hip_gru`: the GRU on csrc/gru.hip with the nn.GRU's own parameters, the
    lengths read on the device in any order, nothing packed).  Not part of the state_dict."""

    def __init__(self, vocab_size, word_emb_dim, hidden_dim):
        super().__init__()
        self.hidden_dim, self.vocab_size, self.word_emb_dim = hidden_dim, vocab_size, word_emb_dim
        self.word_embedding = nn.Sequential(nn.Embedding(vocab_size, word_emb_dim), nn.Tanh())
        self.gru = nn.GRU(word_emb_dim, hidden_dim)
        self.embedding_layer = nn.Sequential(nn.Linear(hidden_dim, 1024), nn.Tanh())
        self.gru_impl = "stock"

    def encode_hidden(self, x, seq_lengths):
        """The GRU's hidden state after each question's last token, [B, hidden_dim], without the embedding layer behind it:
        what the HIP fusion head of VQABaselineNet takes.  From question_gru or the packed stock GRU, as ``gru_impl`` says
        (the stock ``forward`` below does not go through here)."""
        emb = self.word_embedding(x)
        if _hip_gru(self, emb):
            from .gru import question_gru
            rnn = self.gru
            return question_gru(emb, seq_lengths, rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0, rnn.bias_hh_l0)[1]
        lens = seq_lengths.cpu() if torch.is_tensor(seq_lengths) else seq_lengths
        return torch.squeeze(self.gru(pack_padded_sequence(emb, lens, batch_first=True))[1], dim=0)

    def forward(self, x, seq_lengths):
        emb = self.word_embedding(x)
        if _hip_gru(self, emb):                                       # opt-in: csrc/gru.hip, lengths stay on the device
            from .gru import question_gru
            rnn = self.gru
            _, h_last = question_gru(emb, seq_lengths, rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0, rnn.bias_hh_l0)
            return self.embedding_layer(h_last)
        lens = seq_lengths.cpu() if torch.is_tensor(seq_lengths) else seq_lengths
        packed = pack_padded_sequence(emb, lens, batch_first=True)
        _, hidden = self.gru(packed)
        return self.embedding_layer(torch.squeeze(hidden, dim=0))


FUSION_IMPLS = ("stock", "hip")


def _linear_tanh(seq) -> bool:
    return (isinstance(seq, nn.Sequential) and len(seq) == 2 and isinstance(seq[0], nn.Linear) and seq[0].bias is not None
            and isinstance(seq[1], nn.Tanh))


def _hip_fusion(net, f, h) -> bool:
    """Does this forward of the baseline model take the HIP fusion head on `f`, the image encoder's fc7 features, and `h`, the
    GRU's last hidden state?  ``net.fusion_impl``: "stock" (the default: the nn modules) or "hip" (fusion.fusion_head on the
    modules' own parameters: CUDA tensors that are fp32, or any floating type under CUDA autocast, where fusion_head is an
    fp32 island that casts them; a supported shape; a frozen image encoder -- `f` carries no gradient, the head has none for
    it; and the expected structure, ``mlp = [Linear, Dropout, Tanh]``, both ``embedding_layer = [Linear, Tanh]``, fc_final
    a Linear, all with bias.  Everything else takes the stock lines)."""
    impl = net.fusion_impl
    if impl not in FUSION_IMPLS:
        raise ValueError("fusion_impl must be one of %s, got %r" % (FUSION_IMPLS, impl))
    if impl != "hip" or not (f.is_cuda and h.is_cuda) or f.requires_grad:
        return False
    for t in (f, h):
        if t.dtype != torch.float32 and not (t.is_floating_point() and torch.is_autocast_enabled("cuda")):
            return False
    ie, qe, mlp, fc = net.image_encoder.embedding_layer, net.question_encoder.embedding_layer, net.mlp, net.fc_final
    if not (_linear_tanh(ie) and _linear_tanh(qe) and isinstance(fc, nn.Linear) and fc.bias is not None
            and isinstance(mlp, nn.Sequential) and len(mlp) == 3 and isinstance(mlp[0], nn.Linear) and mlp[0].bias is not None
            and isinstance(mlp[1], nn.Dropout) and isinstance(mlp[2], nn.Tanh)):
        return False
    if f.dim() != 2 or h.dim() != 2 or f.shape[0] != h.shape[0] or f.shape[1] != ie[0].in_features \
            or h.shape[1] != qe[0].in_features or ie[0].out_features != qe[0].out_features \
            or mlp[0].in_features != ie[0].out_features or fc.in_features != mlp[0].out_features:
        return False
    from . import fusion
    return fusion.supported(f.shape[0], f.shape[1], h.shape[1], ie[0].out_features, mlp[0].out_features, fc.out_features)


class VQABaselineNet(nn.Module):
    """Element-wise product of image and question embeddings -> MLP -> logits.
    ``fusion_impl``: "stock" (default) or "hip" (`_hip_fusion`: everything behind the VGG and the GRU on csrc/fusion.hip with
    these modules' own parameters; the dropout of ``mlp[1]`` drawn inside the head from ``fusion_dropout_state``, a
    DropoutState, never from torch's generators).  Neither is part of the state_dict."""

    def __init__(self, ques_enc_params, img_enc_params, K):
        super().__init__()
        self.image_encoder = ImageBaselineEncoder(**img_enc_params)
        self.question_encoder = QuestionBaselineEncoder(**ques_enc_params)
        self.mlp = nn.Sequential(nn.Linear(1024, 1000), nn.Dropout(0.5), nn.Tanh())
        self.fc_final = nn.Linear(1000, K)
        self.fusion_impl = "stock"
        self.fusion_dropout_state = None

    def forward(self, x_img, x_ques, x_ques_len):
        if self.fusion_impl != "stock":                               # opt-in: csrc/fusion.hip behind the two encoders
            hip = self._forward_hip(x_img, x_ques, x_ques_len)
            if hip is not None:
                return hip
        joint = self.image_encoder(x_img) * self.question_encoder(x_ques, x_ques_len)
        return self.fc_final(self.mlp(joint))

    def _forward_hip(self, x_img, x_ques, x_ques_len):
        """The logits through fusion.fusion_head, or None where `_hip_fusion` says the stock lines apply (decided on the image
        features, before the question encoder runs: nothing is computed twice)."""
        if self.fusion_impl not in FUSION_IMPLS:
            raise ValueError("fusion_impl must be one of %s, got %r" % (FUSION_IMPLS, self.fusion_impl))
        enc = self.image_encoder
        if not x_img.is_cuda or any(p.requires_grad for p in enc.vgg11_encoder.parameters()):
            return None
        f = enc.vgg11_encoder(x_img)
        h = self.question_encoder.encode_hidden(x_ques, x_ques_len)
        if not _hip_fusion(self, f, h):                               # (the stock tail on what is already there)
            joint = enc.embedding_layer(F.normalize(f, dim=1, p=2)) * self.question_encoder.embedding_layer(h)
            return self.fc_final(self.mlp(joint))
        from .fusion import fusion_head
        p = self.mlp[1].p if self.training else 0.0
        if p > 0 and self.fusion_dropout_state is None:
            raise RuntimeError("VQABaselineNet: fusion_impl = 'hip' with dropout needs fusion_dropout_state (a DropoutState on "
                               "the model's device): train.set_fusion_head(model, 'hip', seed) sets both")
        li, lq, lm, lf = enc.embedding_layer[0], self.question_encoder.embedding_layer[0], self.mlp[0], self.fc_final
        return fusion_head(f, h, li.weight, li.bias, lq.weight, lq.bias, lm.weight, lm.bias, lf.weight, lf.bias,
                           p=p, state=self.fusion_dropout_state, training=self.training)


def set_feature_dropout(model: nn.Module, p: float, seed: int = 0) -> None:
    """Feature dropout of probability `p` on a HierarchicalCoAttentionNet (``model.feature_dropout``), its masks drawn from a
    fresh ``DropoutState(seed)`` on the device the model's parameters are on -- call it after moving the model.  p = 0 switches
    it off and drops the state.  Other models have no such site: p > 0 is an error for them."""
    p = check_p(p)
    if not isinstance(model, HierarchicalCoAttentionNet):
        if p > 0:
            raise ValueError("feature dropout applies to the co-attention models (HierarchicalCoAttentionNet), not to %s"
                             % type(model).__name__)
        return
    model.feature_dropout = p
    model.dropout_state = DropoutState(seed, next(model.parameters()).device) if p > 0 else None
