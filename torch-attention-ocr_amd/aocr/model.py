"""Host-side mirror of the reference's `Model` class (src/model/model.lua:18-731).

Same method names, argument meaning and error behaviour as the Lua class that
src/train.lua drives (`create`, `load`, `step`, `save`, `vis`, `shutdown`, fields
`global_step`, `optim_state.learningRate`), sitting directly on the C ABI of libaocr.
PyTorch is used only as plumbing: device allocations, the HIP stream and
`torch.distributed` (RCCL) for the data-parallel gradient all-reduce.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from types import SimpleNamespace
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib, dist
from ._lib import Config, check, lib, ptr
from .dictionary import edit_distance_device
from .page import backmap_corners, bucket_width, crop_lines_device, crop_lines_slanted_device, rotate_page_device, slant_extent
from .page_pipeline import asked, binarize_stage, binarized_params, clean_stage, colour_stage, flatten_stage, orient_stage, page_boxes, panels_stage, paper, rectify_stage, scale_stage

PAD, GO, EOS = 1, 2, 3
GROUPS = ["cnn", "enc_fw", "enc_bw", "dec", "proj"]

_DEFAULTS = dict(  # src/train.lua:41-62
    dropout=0.0, encoder_num_hidden=512, encoder_num_layers=1, decoder_num_layers=2, target_vocab_size=39,
    target_embedding_size=20, max_encoder_l=80, max_decoder_l=50, input_feed=False, batch_size=400, prealloc=False,
    learning_rate=0.1, seed=910820, img_h=32, max_img_w=100, max_beam=5, compute="f32")


def _cfg_get(config, key):
    if isinstance(config, dict):
        return config.get(key, _DEFAULTS[key])
    return getattr(config, key, _DEFAULTS[key])


def numlist2str(ids):
    """src/utils/utils.lua:119-134."""
    return "".join(chr(v - 1 - 13 + 97) if v > 13 else chr(v - 1 - 3 + 48) for v in ids)


def encoder_columns(W: int) -> np.ndarray:
    """Image column every encoder step is centred on (T = W/4 - 1 steps).  cnn.lua: conv1..conv6 are 3x3 / pad 1 (width kept), the two
    2x2 / stride 2 max-pools after conv1 and conv2 halve it (W/4; the later pools are (2,1) / (1,2) with horizontal stride 1), and conv7 (2x2,
    no pad) makes T = W/4 - 1.  Step t thus reads pooled columns t, t+1, i.e. image columns 4t .. 4t+7, centred at 4t + 4 (0-based, between
    pixels 4t+3 and 4t+4)."""
    T = W // 4 - 1
    return 4.0 * np.arange(max(T, 0), dtype=np.float64) + 4.0


def _cut(row):
    """the ids of a label row up to its first EOS."""
    out = []
    for v in row:
        if v == EOS:
            break
        out.append(int(v))
    return out


def eval_word_err_rate(labels: np.ndarray, target_labels: np.ndarray, visualize: bool = False):
    """evalWordErrRate, src/utils/utils.lua:136-175: sequences are cut at the first EOS (3) and compared exactly."""
    B = labels.shape[0]
    werr, pred, gold = 0.0, [], []
    for b in range(B):
        p, g = _cut(labels[b]), _cut(target_labels[b])
        if visualize:
            pred.append(numlist2str(p)); gold.append(numlist2str(g))
        if p != g:
            werr += 1
    return werr, pred, gold


class Model:
    def __init__(self):
        self._h = None
        self.visualize = False
        self.visualize_file = None
        self.global_step = 0
        self.optim_state = {}
        self.last_norms = None
        self.last_norms_adam = None
        self.optimizer, self.adam_opts, self.adam_state = "sgd", {}, None
        self._comm_stream = None
        self._buckets = None
        self._drop_last_gs, self._drop_repeat = None, 0

    # ------------------------------------------------------------------ construction
    def _set_structure(self, config):
        g = lambda k: _cfg_get(config, k)
        self.cnn_feature_size = 512
        self.dropout = float(g("dropout"))
        if not 0.0 <= self.dropout < 1.0:
            raise ValueError(f"dropout {self.dropout} outside [0, 1)")
        self.dropout_seed = 910820          # the mask is a counter-based function of (seed, global_step, site, element): include/aocr.h
        self.encoder_num_hidden = int(g("encoder_num_hidden"))
        self.encoder_num_layers = int(g("encoder_num_layers"))
        self.decoder_num_hidden = 2 * self.encoder_num_hidden
        self.decoder_num_layers = int(g("decoder_num_layers"))
        self.target_vocab_size = int(g("target_vocab_size"))
        self.target_embedding_size = int(g("target_embedding_size"))
        self.input_feed = bool(g("input_feed"))

    def _set_runtime(self, config):
        g = lambda k: _cfg_get(config, k)
        self.max_encoder_l = int(g("max_encoder_l"))
        self.max_decoder_l = int(g("max_decoder_l"))
        self.batch_size = int(g("batch_size"))
        self.prealloc = bool(g("prealloc"))
        self.img_h = int(g("img_h"))
        self.max_img_w = int(g("max_img_w"))
        self.max_beam = int(g("max_beam"))
        comp = g("compute")
        self.compute = _lib.COMPUTE_BF16 if comp in ("bf16", 1) else _lib.COMPUTE_F32

    def _set_optimizer(self, config):
        """which update `train_step_device` / `step` apply: optimizer="sgd" (the default: optim.sgd_list at optim_state.learningRate, clip 5) or
        "adam" (AdamW, `adam_step`) with adam=dict(lr=, betas=, eps=, weight_decay=, clip=)."""
        get = config.get if isinstance(config, dict) else (lambda k, d=None: getattr(config, k, d))
        opt = get("optimizer", None) or "sgd"
        if opt not in ("sgd", "adam"):
            raise ValueError(f"optimizer={opt!r}: 'sgd' or 'adam'")
        opts = dict(get("adam", None) or {})
        unknown = sorted(set(opts) - {"lr", "betas", "eps", "weight_decay", "clip"})
        if unknown:
            raise ValueError(f"adam={opts!r}: unknown keys {unknown}")
        _lib.AdamParams(**opts)                               # raises ValueError for what the library would turn down
        self.optimizer, self.adam_opts = opt, opts

    def create(self, config):
        """model:create, model.lua:83-112: fresh parameters (Torch7 default init distributions [upstream])."""
        self._set_optimizer(config)
        self._set_structure(config)
        self._set_runtime(config)
        self.global_step = 0
        self.optim_state = {"learningRate": float(_cfg_get(config, "learning_rate"))}
        self._build()
        self._init_parameters(int(_cfg_get(config, "seed")))
        return self

    def load(self, model_path, config=None):
        """model:load, model.lua:45-80: structure from the checkpoint, max_*_l / batch_size from `config`."""
        config = config or {}
        assert os.path.isfile(model_path), f"Model {model_path} does not exist!"
        with open(model_path, "rb") as f:
            magic = f.read(4)
        if magic[:2] != b"PK":                       # not a torch.save zip: a Torch7 file (the reference's checkpoint or our flat export)
            return self._load_t7(model_path, config)
        ck = torch.load(model_path, map_location="cpu", weights_only=True)        # tensors + plain containers only: no pickle execution
        self._set_optimizer(config)
        self._set_structure(ck["config"])
        merged = dict(ck["config"])
        for k in ("max_encoder_l", "max_decoder_l", "batch_size", "prealloc", "img_h", "max_img_w", "max_beam", "compute"):
            v = config.get(k) if isinstance(config, dict) else getattr(config, k, None)
            if v is not None:
                merged[k] = v
        self._set_runtime(merged)
        self.global_step = ck["global_step"]
        self.optim_state = dict(ck["optim_state"])
        self.optim_state.setdefault("learningRate", float(merged.get("learning_rate", _DEFAULTS["learning_rate"])))   # train.lua:87
        self._build()
        self.params.copy_(ck["params"].to(self.params.device))
        self.bn_state.copy_(ck["bn_state"].to(self.params.device))
        self.adam_state = None
        if "adam_state" in ck:                                # AdamW's moments and step bookkeeping (save writes the key only when the state exists)
            st = ck["adam_state"]
            if st.dtype != torch.uint8 or st.numel() != lib.aocr_adam_state_bytes(self.num_params):
                raise ValueError(f"{model_path}: adam_state of {st.numel()} {st.dtype} elements, expected {lib.aocr_adam_state_bytes(self.num_params)} bytes")
            self._adam_alloc().copy_(st.to(self.params.device))
        return self

    def _load_t7(self, model_path, config):
        """model:load on a Torch7-serialized checkpoint (model.lua:51-59): aocr.checkpoint pulls the tensors out of the nets."""
        from .checkpoint import read_t7_checkpoint
        ck = read_t7_checkpoint(model_path)
        self._set_optimizer(config)
        self.adam_state = None                                # the .t7 layouts carry no optimizer state
        merged = dict(_DEFAULTS); merged.update({k: v for k, v in ck["config"].items() if v is not None})
        self._set_structure(merged)
        for k in ("max_encoder_l", "max_decoder_l", "batch_size", "prealloc", "img_h", "max_img_w", "max_beam", "compute"):
            v = config.get(k) if isinstance(config, dict) else getattr(config, k, None)
            if v is not None:
                merged[k] = v
        self._set_runtime(merged)
        self.global_step = ck["global_step"]
        self.optim_state = dict(ck["optim_state"] or {})
        self.optim_state.setdefault("learningRate", float(merged["learning_rate"]))                                  # train.lua:87
        self._build()
        self.set_parameters({k: torch.from_numpy(v) for k, v in ck["params"].items()},
                            {k: torch.from_numpy(v) for k, v in ck["bn_state"].items()})
        return self

    def _build(self):
        """model:_build, model.lua:115-223: flat parameter/gradient vectors + workspace, no cloned cells."""
        if not torch.cuda.is_available():
            raise RuntimeError("aocr.Model needs a HIP device: the hot path has no CPU fallback")
        self.device = torch.device("cuda", torch.cuda.current_device())
        assert self.target_vocab_size <= 40
        self.config = dict(
            dropout=self.dropout, encoder_num_hidden=self.encoder_num_hidden, encoder_num_layers=self.encoder_num_layers,
            decoder_num_hidden=self.decoder_num_hidden, decoder_num_layers=self.decoder_num_layers,
            target_vocab_size=self.target_vocab_size, target_embedding_size=self.target_embedding_size,
            max_encoder_l=self.max_encoder_l, max_decoder_l=self.max_decoder_l, input_feed=self.input_feed,
            batch_size=self.batch_size, prealloc=self.prealloc, img_h=self.img_h, max_img_w=self.max_img_w,
            max_beam=self.max_beam, compute="bf16" if self.compute == _lib.COMPUTE_BF16 else "f32")
        self.ccfg = Config(self.batch_size, self.img_h, self.max_img_w, self.encoder_num_hidden, self.encoder_num_layers,
                           self.decoder_num_layers, self.target_vocab_size, self.target_embedding_size,
                           int(self.input_feed), self.max_decoder_l, self.max_beam, self.compute)
        self.table, self.group_counts = _lib.param_table(self.ccfg)
        self.num_params = sum(self.group_counts)
        self.group_offsets = np.concatenate([[0], np.cumsum(self.group_counts)]).astype(np.int64)
        dev = self.device
        self.params = torch.zeros(self.num_params, dtype=torch.float32, device=dev)       # model.lua:163-168
        self.grad_params = torch.zeros(self.num_params, dtype=torch.float32, device=dev)
        self.bn_state = torch.zeros(lib.aocr_bn_state_count(), dtype=torch.float32, device=dev)
        self._reset_bn_state()
        ws = lib.aocr_workspace_bytes(C.byref(self.ccfg))
        if ws == 0:
            raise _lib.AocrError(_lib.last_error())
        self.workspace = torch.empty(ws, dtype=torch.uint8, device=dev)
        self._scal = torch.zeros(16, dtype=torch.float32, device=dev)                       # loss + norms
        h = C.c_void_p()
        check(lib.aocr_model_create(C.byref(self.ccfg), ptr(self.params), ptr(self.grad_params), ptr(self.bn_state),
                                    ptr(self.workspace), ws, self._stream(), C.byref(h)), "aocr_model_create")
        self._h = h
        self._dec_out = None
        self.init_beam = False

    def _reset_bn_state(self):
        st = torch.zeros_like(self.bn_state)
        o = 0
        for c in (256, 512, 512):
            st[o + c:o + 2 * c] = 1.0           # running_var = 1
            o += 2 * c
        self.bn_state.copy_(st)

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def _init_parameters(self, seed: int):
        gen = torch.Generator().manual_seed(seed)
        host = torch.zeros(self.num_params, dtype=torch.float32)
        for name, group, off, shape in self.table:
            n = int(np.prod(shape))
            leaf = name.split(".")[-1]
            if "conv" in name:
                cout, kh, kw, cin = self._conv_shape(name)
                stdv = 1.0 / math.sqrt(kh * kw * cin)
            elif ".bn" in name:
                stdv = None
            elif name == "dec.lookup":
                stdv = None
            elif len(shape) == 2:                                  # nn.Linear / LinearNoBias weight: 1/sqrt(fan_in)
                stdv = 1.0 / math.sqrt(shape[1])
            else:                                                  # bias: same stdv as its weight
                wshape = next(s for (nm, _, _, s) in self.table if nm == name[:-2] + ".w")
                stdv = 1.0 / math.sqrt(wshape[1])
            if name == "dec.lookup":
                v = torch.randn(n, generator=gen)
            elif ".bn" in name:
                v = torch.rand(n, generator=gen) if leaf == "w" else torch.zeros(n)
            else:
                v = (torch.rand(n, generator=gen) * 2 - 1) * stdv
            host[off:off + n] = v
        self.params.copy_(host.to(self.device))

    def _conv_shape(self, name):
        base = name[:-2]
        return next(s for (nm, _, _, s) in self.table if nm == base + ".w")

    # ------------------------------------------------------------------ parameter import / export (Torch7 layouts)
    def set_parameters(self, named: Dict[str, torch.Tensor], bn_state: Optional[Dict[str, torch.Tensor]] = None):
        """Inject weights given in Torch7 layouts (conv [Cout][Cin][kH][kW], Linear [out][in])."""
        host = torch.zeros(self.num_params, dtype=torch.float32)
        for name, group, off, shape in self.table:
            t = named[name].detach().to(torch.float32).cpu()
            if len(shape) == 4:
                t = t.permute(0, 2, 3, 1).contiguous()           # -> [Cout][kH][kW][Cin]
            assert tuple(t.shape) == tuple(shape), (name, tuple(t.shape), shape)
            host[off:off + t.numel()] = t.reshape(-1)
        self.params.copy_(host.to(self.device))
        if bn_state is not None:
            parts = []
            for i in (3, 5, 7):
                parts += [bn_state[f"cnn.bn{i}.rm"].float().reshape(-1), bn_state[f"cnn.bn{i}.rv"].float().reshape(-1)]
            self.bn_state.copy_(torch.cat(parts).to(self.device))

    def _export(self, flat: torch.Tensor) -> Dict[str, torch.Tensor]:
        host = flat.detach().cpu()
        out = {}
        for name, group, off, shape in self.table:
            n = int(np.prod(shape))
            t = host[off:off + n].reshape(shape)
            if len(shape) == 4:
                t = t.permute(0, 3, 1, 2).contiguous()           # -> Torch7 [Cout][Cin][kH][kW]
            out[name] = t.clone()
        return out

    def get_parameters(self):
        return self._export(self.params)

    def get_gradients(self):
        return self._export(self.grad_params)

    def get_bn_state(self):
        host = self.bn_state.detach().cpu()
        out, o = {}, 0
        for i, c in ((3, 256), (5, 512), (7, 512)):
            out[f"cnn.bn{i}.rm"] = host[o:o + c].clone(); out[f"cnn.bn{i}.rv"] = host[o + c:o + 2 * c].clone()
            o += 2 * c
        return out

    def get_tensor(self, name: str) -> torch.Tensor:
        """parity tap: copy of a named intermediate of the last step."""
        p, nd, shape = C.c_void_p(), C.c_int32(), (C.c_int64 * 4)()
        check(lib.aocr_get_tensor(self._h, name.encode(), C.byref(p), C.byref(nd), shape), "aocr_get_tensor")
        shp = tuple(shape[i] for i in range(nd.value))
        n = int(np.prod(shp))
        off = p.value - self.workspace.data_ptr()                 # every tap lives inside the workspace arena
        assert 0 <= off and off + 4 * n <= self.workspace.numel() and off % 4 == 0
        return self.workspace[off:off + 4 * n].view(torch.float32).reshape(shp).cpu()

    def get_tensor_view(self, name: str, dtype=torch.int32) -> torch.Tensor:
        """A named tap IN PLACE (device view into the workspace, 4-byte elements): tests write the cluster kernels' status word through it."""
        p, nd, shape = C.c_void_p(), C.c_int32(), (C.c_int64 * 4)()
        check(lib.aocr_get_tensor(self._h, name.encode(), C.byref(p), C.byref(nd), shape), "aocr_get_tensor")
        n = int(np.prod([shape[i] for i in range(nd.value)]))
        off = p.value - self.workspace.data_ptr()
        assert 0 <= off and off + 4 * n <= self.workspace.numel() and off % 4 == 0
        return self.workspace[off:off + 4 * n].view(dtype)

    # ------------------------------------------------------------------ one step, model.lua:226-706
    def _upload(self, batch):
        dev = self.device
        images = torch.as_tensor(batch[0]).to(device=dev, dtype=torch.float32).contiguous()     # localize(), utils.lua:96-102
        targets = torch.as_tensor(batch[1]).to(device=dev, dtype=torch.int32).contiguous()
        targets_eval = torch.as_tensor(batch[2]).to(device=dev, dtype=torch.int32).contiguous()
        assert images.dim() == 4 and images.shape[1] == 1 and images.shape[2] == self.img_h
        return images, targets, targets_eval

    def train_step_device(self, images, targets, targets_eval, global_batch=None):
        """One optimisation step on inputs already resident in HBM; enqueues only (no host sync) and returns
        the device scalar holding the step's NLL sum (summed over ranks under data parallelism).
        global_batch: rows of the step over ALL ranks (default: this rank's rows x world size, i.e. equal slices)."""
        B, _, _, W = images.shape
        target_l = targets.shape[1]
        assert target_l <= self.max_decoder_l, f"max_decoder_l ({self.max_decoder_l}) < target_l ({target_l})!"
        check(lib.aocr_model_set_stream(self._h, self._stream()))
        loss_dev = self._scal[0:1]
        if dist.world_size() > 1 and not os.environ.get("AOCR_PY_EXCHANGE"):
            dist.attach(self, sync_bn=not os.environ.get("AOCR_NO_SYNC_BN"))       # once: torch.distributed becomes the library's provider
        # d(loss) / (global batch): model.lua:645-647 divides by the step's batch size
        scale = dist.grad_scale(B) if global_batch is None else 1.0 / float(global_batch)
        self._arm_dropout()
        check(lib.aocr_train_forward_backward(self._h, ptr(images), ptr(targets), ptr(targets_eval), B, W, target_l,
                                              scale, ptr(loss_dev)), "aocr_train_forward_backward")
        # the one exchange step of data parallelism (RCCL over xGMI), between feval and the per-group clip; bucketed in the order
        # the backward pass completes the gradient vector and run on a second stream beside it
        if getattr(self, "_comm_cb", None) is not None or getattr(self, "_comm_rccl", False):
            check(lib.aocr_allreduce_grads(self._h, ptr(loss_dev)), "aocr_allreduce_grads")   # inside the library (include/aocr.h)
        elif dist.world_size() > 1 and os.environ.get("AOCR_NO_OVERLAP"):
            dist.exchange(self.grad_params, loss_dev)             # one all-reduce after the backward pass (A/B against the overlap)
        elif dist.world_size() > 1:
            if self._comm_stream is None:
                self._comm_stream = torch.cuda.Stream(device=self.device)
                self._buckets = dist.bucket_ranges(self.ccfg)
            dist.exchange_overlapped(self.grad_params, loss_dev, self._buckets, self._wait_bucket, self._comm_stream)
        if dist.world_size() > 1 and getattr(self, "_comm_cb", None) is None and not getattr(self, "_comm_rccl", False):
            self._exchange_timeout_flag()
        if self.optimizer == "adam":
            self.adam_step(**self.adam_opts)
            return loss_dev
        norms = self._scal[2:12]
        check(lib.aocr_sgd_step(self._h, float(self.optim_state["learningRate"]), 5.0, ptr(norms)), "aocr_sgd_step")
        self.last_norms = norms
        return loss_dev

    def _exchange_timeout_flag(self):
        """Host-side exchange paths (AOCR_PY_EXCHANGE): a caller that sums the gradient buckets itself must also make the cluster
        kernels' time-out code a GLOBAL decision, as aocr_allreduce_grads does inside the library (include/aocr.h, aocr_cluster_status):
        MAX over ranks of the status word, so every rank's optimizer skips (or applies) the update together."""
        try:
            flag = self.get_tensor_view("cl_err")[0:1]
        except RuntimeError:
            return                                                # configuration without whole-sequence kernels: nothing can time out
        torch.distributed.all_reduce(flag, op=torch.distributed.ReduceOp.MAX)

    def _wait_bucket(self, k, stream):
        check(lib.aocr_stream_wait_grads(self._h, k, C.c_void_p(stream.cuda_stream)), "aocr_stream_wait_grads")

    def decode_device(self, images, targets, targets_eval, beam_size=1, trie=None):
        """forward_only feval on device-resident inputs; enqueues only.  Returns device tensors
        (labels (B,max_decoder_l) int32, beam scores (B), gold scores (B), gold-pass NLL sum (1)).
        trie: an `aocr.dictionary.Trie` already on this device (-use_dictionary, model.lua:380-387,405-445,460-513) or None."""
        B, _, _, W = images.shape
        Lt = self.max_decoder_l
        check(lib.aocr_model_set_stream(self._h, self._stream()))
        labels = torch.empty((B, Lt), dtype=torch.int32, device=self.device)
        scores = torch.empty(B, dtype=torch.float32, device=self.device)
        gold = torch.empty(B, dtype=torch.float32, device=self.device)
        loss_dev = self._scal[0:1]
        if trie is None:
            check(lib.aocr_decode(self._h, ptr(images), ptr(targets), ptr(targets_eval), B, W, targets.shape[1], beam_size,
                                  ptr(labels), ptr(scores), ptr(gold), ptr(loss_dev)), "aocr_decode")
        else:
            desc = trie.desc()
            check(lib.aocr_decode_dict(self._h, ptr(images), ptr(targets), ptr(targets_eval), B, W, targets.shape[1], beam_size,
                                       C.byref(desc), ptr(labels), ptr(scores), ptr(gold), ptr(loss_dev)), "aocr_decode_dict")
        return labels, scores, gold, loss_dev

    def recognize_device(self, images, beam_size=1, trie=None, attention=False, char_scores=False):
        """Label-free recognition (aocr_recognize) of a preprocessed (B,1,32,W) batch already in HBM; enqueues only.  Returns device tensors
        (labels (B,max_decoder_l) int32, scores (B), char_logp (B,max_decoder_l) or None, attention (B,max_decoder_l,T) or None, T = W/4 - 1).
        labels / scores are what decode_device returns for the same images; no targets, no gold pass."""
        B, _, _, W = images.shape
        Lt = self.max_decoder_l
        T = W // 4 - 1
        check(lib.aocr_model_set_stream(self._h, self._stream()))
        labels = torch.empty((B, Lt), dtype=torch.int32, device=self.device)
        scores = torch.empty(B, dtype=torch.float32, device=self.device)
        clp = torch.empty((B, Lt), dtype=torch.float32, device=self.device) if char_scores else None
        attn = torch.empty((B, Lt, max(T, 1)), dtype=torch.float32, device=self.device) if attention else None
        desc = None
        if trie is not None:
            if trie._dev is None:
                trie.to(self.device)
            desc = trie.desc()
        check(lib.aocr_recognize(self._h, ptr(images), B, W, beam_size, C.byref(desc) if desc is not None else None, ptr(labels), ptr(scores),
                                 ptr(clp), ptr(attn)), "aocr_recognize")
        return labels, scores, clp, attn

    def recognize(self, images, beam_size=None, trie=None, attention=False, width=None, lexicon=None, lexicon_rows=None):
        """Read images without labels.  images: a preprocessed (B,1,32,W) tensor, or a list of uint8 (H,W) / (H,W,3) arrays (load_image), which
        go through preprocess_batch at `width` (default max_img_w).  Returns a namespace: labels (B,max_decoder_l) int32, scores (B), text (per
        row, cut at the first EOS), char_logp (B,max_decoder_l), attention (B,max_decoder_l,T) when asked for (else None) and columns (T): the
        image column every encoder step is centred on.
        lexicon: an `aocr.Lexicon`; every row is also snapped to its nearest word (aocr_lexicon_nearest) and the namespace carries word (per row,
        None for an empty range), word_index (B) and word_distance (B) int32.  lexicon_rows (B+1): row b searches the words
        [lexicon_rows[b], lexicon_rows[b+1]) of the lexicon (per-image lexicons); None: the whole list."""
        if lexicon is None and lexicon_rows is not None:
            raise ValueError("lexicon_rows without a lexicon")
        if isinstance(images, (list, tuple)):
            from .data import preprocess_batch
            images = preprocess_batch(list(images), int(width or self.max_img_w), self.device, self._stream())
        else:
            images = torch.as_tensor(images).to(device=self.device, dtype=torch.float32).contiguous()
        assert images.dim() == 4 and images.shape[1] == 1 and images.shape[2] == self.img_h
        beam_size = min(beam_size or 1, self.target_vocab_size)
        labels, scores, clp, attn = self.recognize_device(images, beam_size, trie, attention, True)
        snapped = None
        if lexicon is not None:
            if lexicon._dev is None or lexicon._dev.device != self.device:
                lexicon.to(self.device)
            snapped = lexicon.nearest(labels, lexicon_rows, self._stream())
        labels_h = labels.cpu().numpy()
        text = [numlist2str(_cut(row)) for row in labels_h]
        self.check_health()
        res = SimpleNamespace(labels=labels_h, scores=scores.cpu().numpy(), text=text, char_logp=clp.cpu().numpy(),
                              attention=attn.cpu().numpy() if attn is not None else None, columns=encoder_columns(images.shape[3]))
        if snapped is not None:
            res.word_index, res.word_distance = snapped[0].cpu().numpy(), snapped[1].cpu().numpy()
            res.word = [lexicon.words[i] if i >= 0 else None for i in res.word_index.tolist()]
        return res

    def _page_boxes(self, page, stream, seg, max_boxes, deskew, dewarp, layout, clean_dev, colour_dev=None, deslant=None, spacing=None, rules=None,
                    panels_dev=None, binarize_dev=None):
        """the middle of recognize_page (aocr.page_pipeline.page_boxes), reached through the model so that a caller can wrap it."""
        return page_boxes(page, stream, seg, max_boxes, deskew, dewarp, layout, clean_dev, colour_dev, deslant, spacing, rules, panels_dev,
                          binarize_dev)

    def recognize_page(self, page, params=None, width=None, width_step=32, beam_size=1, trie=None, lexicon=None, max_boxes=1024, deskew=None, flatten=None,
                       layout=None, clean=None, orient=None, rectify=None, scale=None, dewarp=None, colour=None, deslant=None, spacing=None,
                       panels=None, binarize=None, rules=None):
        """Read a scanned page: segment it into word boxes (aocr_segment_page), crop them (aocr_crop_lines) and recognise the crops.
        page: a uint8 (H,W) numpy array or tensor (gray; a 3-D array raises ValueError unless `colour` is asked for: see below).  params: an
        `aocr.SegmentParams` (default: Otsu threshold, dark text).  The counts and boxes are read back once (the one sync), then the boxes are
        bucketed by crop width: `width` an int gives one bucket; otherwise each box gets DataGen's width rule (aocr.page.bucket_width with
        width_step, capped at max_img_w).  Every bucket is cropped and recognised in chunks of at most batch_size rows through
        recognize_device and, with a lexicon, Lexicon.nearest.
        Returns a namespace in reading order (line, then x): boxes (n,4) int32 x0 y0 x1 y1, line (n), ink (n), text, labels (n,max_decoder_l),
        scores (n), widths (n), threshold, n_found, n_lines, truncated (n_found > max_boxes), and word / word_index / word_distance with a
        lexicon.  A page without boxes gives empty arrays.
        deskew: None (the default) segments the page as it is.  True or an `aocr.SkewParams` first estimates the slope of the lines
        (aocr_estimate_skew; True: the default sweep with the threshold and light_text of `params`) and shears it out (aocr_deskew_page, filled
        with paper: 0 with light_text, else 255), then segments, crops and recognises the deskewed page, all enqueued on the same stream; the
        skew words come back with the counts (still one sync).  The namespace then also carries skew_steps, skew_slope_q16, skew_deg
        (atan(slope / 65536) in degrees) and source_corners (n,4,2): the (x, y) of every box's corner pixels on the page as given
        (aocr.page.source_corners); boxes are in deskewed-page coordinates.
        flatten: None or False (the default) reads the page as it is.  True or an `aocr.FlattenParams` first divides the page's background out
        (aocr_flatten_page; True: radius 16 with the light_text of `params`), for a page whose paper is not evenly lit; the skew estimate, the
        deskew, the segmentation and the crops then all read the flattened page.  Enqueued on the same stream, still one sync.  The namespace
        then also carries flatten_radius.
        layout: None or False (the default) segments the page as one column.  True or an `aocr.LayoutParams` reads a multi-column page: after
        flatten and deskew the page's ink table and its recursive XY cut are enqueued (aocr_ink_integral, aocr_layout_blocks, at most 256
        blocks, with the threshold and light_text of `params`), and the blocks, their counts and the page threshold are read back (the skew
        comes with them): the FIRST sync.  Every block is then segmented as a view of the page (aocr_segment_page with the page threshold, so
        Otsu is not redone per block; max_boxes applies per block and the padding clamps to the block), the boxes are shifted to page
        coordinates and the line numbers continued across blocks on the device, and all counts and boxes are read back together: the SECOND
        sync (this path has two, the others one).  Crops are taken from the whole page.  The namespace is in reading order (block, then
        line, then x) and also carries block (n): the block of every box, blocks (m,4) x0 y0 x1 y1, block_depth (m), n_blocks and
        layout_overflow; truncated is true when any block truncated.
        clean: None or False (the default) reads the page as it is.  True or an `aocr.CleanParams` first paints over the connected components of
        the ink that cannot be text (aocr_clean_page: specks and rules; True: the defaults with the threshold and light_text of `params`),
        after flatten and before deskew; everything after it reads the cleaned page.  Enqueued on the same stream; its eight counts come back
        with the existing readback (one sync, two with layout).  The namespace then also carries clean_components, clean_specks, clean_rules
        and clean_ink_removed.
        orient: None or False (the default) reads the page as it is.  An int 0..3 first turns the page by that many clockwise quarter turns
        (aocr_rotate_page), after flatten and clean and before deskew: no estimate and no extra sync.  True is automatic: the run starts of
        the ink are counted along x and along y (aocr_estimate_orientation, with the threshold and light_text of `params`) and read back -- ONE
        ADDITIONAL sync, which cannot be avoided because the page's shape may change -- and the page is turned by the quarter turn they
        propose.  The counts cannot tell a page from the same page upside down, so the recogniser is asked: after deskew, layout and
        segmentation the first min(n, batch_size) boxes are cropped at one width (`width`, or the widest bucket among them) and recognised
        twice, as cropped and turned by a half turn (torch.flip of the crop batch: a few small crops, not the page); when the flipped crops'
        mean score is strictly higher, the page is turned by a further half turn and deskew, layout, segmentation and recognition start over
        on it.  The namespace then also carries orientation (the clockwise quarter turns applied in all), orient_runs ((N_h, N_v); None
        unless automatic), orient_scores ((mean score as cropped, flipped) of the probe, (0.0, 0.0) for a page without boxes; None unless
        automatic) and source_boxes (n,4): the boxes on the page as given (aocr.page.unrotate_boxes); boxes are in the coordinates of the
        page that was segmented, and with deskew source_corners goes through the shear and then the rotation back to the page as given.
        Limits of the estimate (thin margins, pages of digits): DESIGN.md section 17.
        rectify: None or False (the default) reads the page as it is.  Anything else treats the page as a photograph, a sheet of paper lying
        on a desk and seen in perspective, and straightens it FIRST, before flatten: flatten would divide the desk out to paper, and no later
        stage could then tell the two apart.  True or an `aocr.RectifyParams` finds the paper's corners on the device (aocr_find_page_quad:
        the extremes along the diagonals of the largest component on the paper side of an Otsu threshold; True: dark_paper = the light_text
        of `params`) and reads the 16 words back -- ONE ADDITIONAL sync, which cannot be avoided because the corners set the shape of the
        page that every later stage reads.  When the quad is valid and the sheet covers at least min_area_percent of the photograph, the
        output size and the coefficients are planned on the host (aocr_rectify_plan) and the page is resampled (aocr_warp_page, filled with
        paper: 0 with light_text, else 255); otherwise the page is used as it is.  A sequence of four (x, y) corners in the order TL, TR,
        BR, BL is used as given: no estimate and no extra sync; a quad that is not convex and clockwise raises ValueError.  The namespace
        then also carries rectified (bool), rectify_quad ((4,2) int, None when no sheet was found), rectify_size ((Wo, Ho), None unless
        rectified), rectify_area (the sheet's pixels, None for corners given) and photo_corners (n,4,2) float64: the corner pixels of every
        box -- source_corners with deskew, those of source_boxes with orient, else those of boxes -- carried back onto the photograph
        (aocr.page.warp_points).  Limits (sheets turned by 45 degrees or more, dog ears, a desk as bright as the paper): DESIGN.md
        section 18.
        scale: None or False (the default) reads the page at the resolution it has.  Anything else resamples it, after flatten and before
        clean, so that its text has the size the other stages' pixel defaults were written for (min_line_h, word_gap, gap_x, min_area ...:
        text at 300 dpi).  True or an `aocr.ScaleParams` measures the glyphs on the device (aocr_estimate_glyph_size: the median of min(w, h)
        over the component boxes; True: the threshold and light_text of `params`) and reads the 8 words back -- ONE ADDITIONAL sync, which
        cannot be avoided because the size sets the shape of the page that every later stage reads; aocr.scale_plan then picks the output size
        (none when the text is within the tolerance of the target, or too few glyphs qualified) and aocr_resize_page resamples by exact pixel
        areas.  A positive number is the ratio to resample by (0.5 halves both sides): no estimate and no extra sync.  The namespace then also
        carries scaled (bool), scale_size (the median, None for a ratio given), scale_quartiles ((q_1, q_3), None likewise), scale_glyphs
        (how many components qualified, None likewise), scale_shape ((Wo, Ho), None unless scaled) and unscaled_corners (n,4,2) float64: the
        corner pixels of every box -- source_corners with deskew, those of source_boxes with orient, else those of boxes -- on the page as it
        was before resizing, xs = (x + 0.5) * W / Wo - 0.5 (aocr.page.unscale_points); with rectify, photo_corners goes through this map
        first.  Limits (a median of boxes, not an x-height; below about 4 pixels the estimate is noise): DESIGN.md section 19.
        dewarp: None or False (the default) reads the page as it is.  True or an `aocr.CurlParams` takes out page curl -- the curved text
        lines of a page bending into a book's gutter, which a shear cannot straighten -- after the deskew and before layout and segmentation
        (so an orient=True half-turn restart redoes it): the row shift of every group of columns against the middle group is estimated
        (aocr_estimate_curl; True: groups of 128 columns, shifts up to 8 rows, the threshold and light_text of `params`) and every column is
        moved back by its interpolated shift (aocr_dewarp_page, filled with paper: 0 with light_text, else 255); the shifts go from one to
        the other on the device, and the curl words and shifts come back with the existing readback (no additional sync).  The namespace
        then also carries curl_shifts (ng) int32, curl_group, curl_max (the largest |shift|), curl_pairs (the pairs of neighbouring groups
        with a non-zero shift) and uncurled_corners (n,4,2) float64: every box's corner pixels on the page that the dewarp read
        (aocr.page.uncurl_points: x stays, y moves by the column's shift); boxes are in dewarped-page coordinates.  source_corners,
        photo_corners and unscaled_corners then start from uncurled_corners with y rounded half up (floor(y + 0.5)); source_boxes stays an
        axis-aligned box and ignores the curl.  Limits (max_shift against the line pitch, errors adding up along the chain, empty margins,
        no foreshortening): DESIGN.md section 20.
        colour: None or False (the default) takes a gray page, and a 3-D page raises ValueError.  Anything else takes a colour page, a uint8
        (H, W, 3) RGB array or tensor as aocr.data.load_image returns it for a colour file (anything else then raises ValueError), and
        reduces it to gray on the device FIRST, before rectify (aocr_estimate_page_colour, aocr_gray_page): the colour of the paper is
        estimated and divided out of every channel, so that yellowed paper or warm light costs no contrast, and the gray value is the luma
        of the balanced pixel.  An `aocr.ColourParams` is used as given: with drop, the coloured pixels of the chosen hue classes (a red
        form rule, a highlighter stroke, a blue stamp: 1 << aocr.HUE_RED ...) become fill before any threshold or profile sees them; mode 1
        takes the darkest channel instead, so that coloured ink comes out dark.  True: the defaults, nothing dropped, fill = paper (0 with
        light_text, else 255), and with light_text no balancing.  The shape does not change, so boxes and corner fields are unaffected; the
        sixteen colour words come back with the existing readback (no additional sync).  The namespace then also carries colour_paper (the
        three paper values divided out), colour_balanced (whether the page was balanced: the params' balance), colour_hues (6) int64: the coloured pixels
        of the classes RED, YELLOW, GREEN, CYAN, BLUE, MAGENTA, and colour_dropped (the pixels replaced by fill).  Limits (a desk larger
        than the sheet wins the paper estimate; coloured text goes with coloured marks of its class): DESIGN.md section 21.
        deslant: None or False (the default) crops the boxes as they are.  True or an `aocr.SlantParams` takes the lean of italic print and
        handwriting out of every crop: right after the segmentation, on the page that was segmented, one slant per box is estimated on the
        device (aocr_estimate_slant: a sweep of sheared column profiles; True: +-12 steps of 1/16 column per row with the light_text of
        `params`; the threshold is the word the segmentation left on the device, with layout the page threshold already read back, the
        estimate then running per block), and the slant words come back inside the readback of the boxes (no additional sync).  Every box
        is bucketed by (w + 2D, h), D = aocr.page.slant_extent, and cropped with its rows moved back along x (aocr_crop_lines_slanted, filled
        with paper: 0 with light_text, else 255); the which-way-up probe of orient=True keeps the plain crops.  The namespace then also
        carries slant_q16 (n) int32, slant_deg (n) float64 (atan(s / 65536) in degrees), slant_flags (n) int32 (0 estimated, 1 taller than
        256 rows and left alone, 2 empty) and slant_extent (n) int32; boxes and every *_corners field stay what they are: the boxes do not
        move.  Limits (any vertical alignment scores, one round glyph has no slant, one slant per box): DESIGN.md section 22.
        spacing: None or False (the default) cuts every line into words with the one word_gap of `params`.  True or an `aocr.SpacingParams`
        estimates the word gap of every line on the device from the line's own gaps between ink-column runs (aocr_segment_page_spaced in
        place of aocr_segment_page, per block with layout: Otsu's split of the gap lengths, clamped to a share of the line height; word_gap
        is then not read, but 0 is an error), so that a headline, body text and a footnote on one page are each cut by their own gap.
        The spacing rows come back inside the readback of the boxes (no additional sync).  The namespace then also carries word_gaps
        (n_lines) int32, the gap used per line, spacing_flags (n_lines) int32 (0 estimated, 1 too few gaps, 2 one gap length, 3 classes
        not separated: the share of the line height was used; + 4 clamped) and spacing_gaps (n_lines) int32, the gaps counted; with
        layout they run across the blocks like the line numbers.  Limits (justified text, lines of one or two words, digits with wide
        tracking, the band height as the em): DESIGN.md section 23.
        rules: None or False (the default) reads the page with its rules.  True or an `aocr.RuleParams` takes the rules of a form or a table
        out and keeps the text that touches them (aocr_remove_rules: per pixel, from run lengths -- a rule is long one way and thin the
        other, a stroke that crosses it is not thin; True: both axes, runs of 100 pixels at most 6 thick, edge 1, with the threshold and
        light_text of `params`: a judgement for 300 dpi, untuned), after deskew and dewarp (a rule is a pure row run only on a straight
        page; an orient=True half-turn restart redoes it) and before layout and segmentation; layout, segmentation and the crops read the
        page with the rules taken out.  The boxes do not move, so every *_corners field stays what it is.  The eight counts come back with
        the existing readback (no additional sync).  The namespace then also carries rules_counts (8) int64 (threshold, total ink, erased,
        crossings, of horizontal rules, of vertical rules, candidates kept, 0), rules_erased and rules_kept.  With clean: clean runs earlier
        and still deletes a grid higher than its max_h together with what touches it: for forms pass clean=aocr.CleanParams(max_h=0) (specks
        only) together with rules=True.  Limits (rules thicker than max_thick, dashed leaders, pages not deskewed, letter bottoms within
        `edge` of a rule they sit on, long thin headline strokes): DESIGN.md section 24.
        panels: None or False (the default) reads the page with one polarity, that of `params`.  True or an `aocr.PanelParams` first finds
        the reversed-out panels -- table header rows, section bars, banners, sidebar boxes: light text on a dark slab -- and inverts the
        bytes inside them (aocr_invert_panels: a connected component whose box is at least min_w x min_h, that fills at least
        fill_percent of its row-convex hull and has at least min_inside_percent of the hull not ink; True: 64 x 24, 60 %, 2 %, with the
        threshold and light_text of `params`: a judgement for 300 dpi, untuned), after scale and before clean, which would otherwise
        paint the slab over as a figure, words and all; every later stage reads the page with the slabs inverted.  At most 256
        candidates are examined.  The boxes do not move, so every *_corners field stays what it is.  The counts and the panel rows come
        back with the existing readback (no additional sync).  The namespace then also carries panels (n, 8) int32, one row x0 y0 x1 y1
        label area hull accepted per examined candidate in label order, in the coordinates of the page after the scale stage (before
        any quarter turn, deskew or dewarp), and panel_counts (8) int64 (components, candidates found, candidates examined, panels
        inverted, threshold, total ink, the sum of the inverted hulls, 0).  Limits (one level of nesting, gray rim pixels, solid bars,
        slabs that touch a grid): DESIGN.md section 26.
        binarize: None or False (the default) separates ink from paper with one threshold for the whole page.  True or an
        `aocr.BinarizeParams` first thresholds every pixel against the mean and the standard deviation of the window around it
        (aocr_binarize_page, Sauvola; True: radius 20, k = 51 / 256, R = 128, gray output, with the light_text of `params`: a judgement
        for 300 dpi, untuned), directly after flatten and before scale, for faded print beside strong print, stains, show-through and
        carbon copies, where no single gray level is right everywhere.  On its output the fixed threshold 127 is the local decision, so
        when `params` asks for Otsu (-1) every later stage runs with 127 on a copy of `params` (the caller's object is not modified, and
        res.threshold is then 127); a fixed threshold in `params` is kept.  The boxes do not move.  The four count words come back with
        the existing readback (no additional sync).  The namespace then also carries binarize_radius, binarize_ink (the ink pixels of the
        local decision) and binarize_threshold_range (the smallest and the largest local T).  Limits (strokes wider than the window are
        hollowed out; it does not replace flatten for strong shading: the two compose, flatten first): DESIGN.md section 27."""
        if asked(colour):
            ok = isinstance(page, (np.ndarray, torch.Tensor)) and len(page.shape) == 3 and page.shape[2] == 3 and \
                page.dtype == (np.uint8 if isinstance(page, np.ndarray) else torch.uint8)
            if not ok:
                raise ValueError(f"colour={colour!r}: page must be a uint8 (H, W, 3) RGB array or tensor, got {getattr(page, 'dtype', type(page))} "
                                 f"{tuple(getattr(page, 'shape', ()))}")
            if not (colour is True or isinstance(colour, _lib.ColourParams)):
                raise ValueError(f"colour={colour!r}: None, False, True or an aocr.ColourParams")
            if isinstance(page, np.ndarray):
                page = torch.from_numpy(np.ascontiguousarray(page))
            seg = params if params is not None else _lib.SegmentParams()
            page, colour_dev, colour_used = colour_stage(page.to(self.device), self._stream(), seg, colour)
        else:
            colour_dev = None
        if isinstance(page, np.ndarray):
            if page.ndim != 2 or page.dtype != np.uint8:
                raise ValueError(f"page must be a uint8 (H, W) array, got {page.dtype} {page.shape}: colour pages are out of scope")
            page = torch.from_numpy(np.ascontiguousarray(page))
        page = torch.as_tensor(page)
        if page.dim() != 2 or page.dtype != torch.uint8:
            raise ValueError(f"page must be a uint8 (H, W) tensor, got {page.dtype} {tuple(page.shape)}: colour pages are out of scope")
        page = page.to(self.device)
        beam_size = min(beam_size or 1, self.target_vocab_size)
        stream = self._stream()
        seg = params if params is not None else _lib.SegmentParams()
        page, rect = rectify_stage(page, stream, seg, rectify)
        page, flat = flatten_stage(page, stream, seg, flatten)
        page, binar, binarize_dev = binarize_stage(page, stream, seg, binarize)
        if binar is not None:
            seg = binarized_params(seg)
        page, scl = scale_stage(page, stream, seg, scale)
        page, panels_dev = panels_stage(page, stream, seg, panels)
        page0, clean_dev = clean_stage(page, stream, seg, clean)
        page, quarter, orient_runs = orient_stage(page0, stream, seg, orient)
        middle = (stream, seg, max_boxes, deskew, dewarp, layout, clean_dev) + (() if colour_dev is None else (colour_dev,))
        extra = dict(deslant=deslant) if asked(deslant) else {}
        if asked(spacing):
            extra["spacing"] = spacing
        if asked(rules):
            extra["rules"] = rules
        if panels_dev is not None:
            extra["panels_dev"] = panels_dev
        if binarize_dev is not None:
            extra["binarize_dev"] = binarize_dev
        st = self._page_boxes(page, *middle, **extra)
        orient_scores = None
        if orient is True:
            m = min(st.n, self.batch_size)                          # which way up: the recogniser reads the first boxes both ways
            orient_scores = (0.0, 0.0)
            if m:
                r = st.rows[:m]
                pw = int(width) if width is not None else max(bucket_width(int(b[2] - b[0]), int(b[3] - b[1]), self.max_img_w, width_step) for b in r)
                crops = crop_lines_device(st.page, st.boxes_dev[:m], None, pw, self.img_h, stream)
                up = self.recognize_device(crops, beam_size, trie)[1].mean()
                down = self.recognize_device(torch.flip(crops, (2, 3)).contiguous(), beam_size, trie)[1].mean()
                orient_scores = tuple(float(v) for v in torch.stack([up, down]).cpu().numpy())
            if orient_scores[1] > orient_scores[0]:
                quarter = (quarter + 2) & 3
                st = self._page_boxes(rotate_page_device(page0, quarter, None, stream), *middle, **extra)
        page, rows, counts, n = st.page, st.rows, st.counts, st.n
        extent = slant_extent(rows, st.slant[:, 1]) if st.slant is not None else np.zeros(n, np.int32)
        if width is not None:
            widths = np.full(n, int(width), np.int64)
        else:
            widths = np.array([bucket_width(int(r[2] - r[0]) + 2 * int(d), int(r[3] - r[1]), self.max_img_w, width_step)
                               for r, d in zip(rows, extent)], np.int64).reshape(n)
        labels = np.full((n, self.max_decoder_l), PAD, np.int32)
        scores = np.zeros(n, np.float32)
        word_index, word_distance = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
        if lexicon is not None and (lexicon._dev is None or lexicon._dev.device != self.device):
            lexicon.to(self.device)
        for w in sorted(set(widths.tolist())):
            members = np.nonzero(widths == w)[0]
            for c0 in range(0, len(members), self.batch_size):
                idx = members[c0:c0 + self.batch_size]
                idx_dev = torch.from_numpy(idx).to(self.device)
                sel = st.boxes_dev[idx_dev]
                if st.slant_dev is None:
                    crops = crop_lines_device(page, sel, None, int(w), self.img_h, stream)
                else:
                    crops = crop_lines_slanted_device(page, sel, None, st.slant_dev[idx_dev], int(w), self.img_h, paper(seg), stream)
                lab, sc, _, _ = self.recognize_device(crops, beam_size, trie)
                if lexicon is not None:
                    wi, wd = lexicon.nearest(lab, None, stream)
                    word_index[idx], word_distance[idx] = wi.cpu().numpy(), wd.cpu().numpy()
                labels[idx], scores[idx] = lab.cpu().numpy(), sc.cpu().numpy()
        if n:
            self.check_health()
        text = [numlist2str(_cut(row)) for row in labels]
        res = SimpleNamespace(boxes=rows[:, :4].copy(), line=rows[:, 4].copy(), ink=rows[:, 5].copy(), text=text, labels=labels, scores=scores,
                              widths=widths, threshold=int(counts[2]), n_found=int(counts[0]), n_lines=int(counts[1]),
                              truncated=st.truncated)
        if st.lay is not None:
            res.block, res.blocks, res.block_depth = st.block_id, st.blocks[:, :4].copy(), st.blocks[:, 4].copy()
            res.n_blocks, res.layout_overflow = st.nb, bool(st.lcounts[3])
        if flat is not None:
            res.flatten_radius = int(flat.radius)
        if binar is not None:
            res.binarize_radius, res.binarize_ink = int(binar.radius), int(st.binarize[0])
            res.binarize_threshold_range = (int(st.binarize[1]), int(st.binarize[2]))
        if st.cleaned is not None:
            res.clean_components, res.clean_specks, res.clean_rules, res.clean_ink_removed = (int(st.cleaned[0]), int(st.cleaned[1]),
                                                                                              int(st.cleaned[2]), int(st.cleaned[5]))
        if st.colour is not None:
            res.colour_paper, res.colour_balanced = tuple(int(v) for v in st.colour[:3]), bool(colour_used.balance)
            res.colour_hues, res.colour_dropped = st.colour[4:10].astype(np.int64), int(st.colour[10])
        if st.slant is not None:
            res.slant_q16, res.slant_flags, res.slant_extent = st.slant[:, 1].astype(np.int32), st.slant[:, 2].astype(np.int32), extent
            res.slant_deg = np.degrees(np.arctan(res.slant_q16 / 65536.0))
        if st.spacing is not None:
            res.word_gaps, res.spacing_flags, res.spacing_gaps = (st.spacing[:, k].astype(np.int32) for k in range(3))
        if st.rules is not None:
            res.rules_counts = st.rules.astype(np.int64)
            res.rules_erased, res.rules_kept = int(st.rules[2]), int(st.rules[6])
        if st.panels is not None:
            res.panel_counts = st.panels[:8].astype(np.int64)
            res.panels = st.panels[8:].reshape(-1, 8)[:int(st.panels[2])].astype(np.int32)
        curl = skew = turn = None                                   # what each stage left behind for aocr.page.backmap_corners
        if st.curl is not None:
            res.curl_shifts, res.curl_group = st.curl[4:].astype(np.int32), st.curl_group
            res.curl_max, res.curl_pairs = int(st.curl[1]), int(st.curl[3])
            curl = res.curl_shifts, res.curl_group
        if st.skew is not None:
            res.skew_steps, res.skew_slope_q16 = int(st.skew[0]), int(st.skew[1])
            res.skew_deg = math.degrees(math.atan(res.skew_slope_q16 / 65536.0))
            skew = res.skew_slope_q16, page.shape[0], page.shape[1]
        if quarter is not None:
            res.orientation, res.orient_runs, res.orient_scores = quarter, orient_runs, orient_scores
            turn = quarter, int(page0.shape[0]), int(page0.shape[1])
        if scl is not None:
            res.scaled, res.scale_size, res.scale_quartiles, res.scale_glyphs, res.scale_shape = (scl.shape is not None, scl.size, scl.quartiles,
                                                                                                  scl.glyphs, scl.shape)
        if rect is not None:
            res.rectified, res.rectify_quad, res.rectify_size, res.rectify_area = rect.used, rect.quad, rect.size, rect.area
        vars(res).update(backmap_corners(res.boxes, curl, skew, turn, None if scl is None else scl.resize, None if rect is None else rect.warp))
        if lexicon is not None:
            res.word_index, res.word_distance = word_index, word_distance
            res.word = [lexicon.words[i] if i >= 0 else None for i in word_index.tolist()]
        return res

    def profile_kernel(self, which=0, iters=20):
        """HIP-event timing of one hot kernel at the last step's shape: (ms per launch, flops per launch)."""
        ms, fl = C.c_float(), C.c_double()
        check(lib.aocr_profile_kernel(self._h, which, iters, C.byref(ms), C.byref(fl)), "aocr_profile_kernel")
        return ms.value, fl.value

    def profile_families(self, fn, repeats=3):
        """Per-family HIP-event timing (include/aocr.h AOCR_PROF_*): runs fn() `repeats` times with the library's marks on and
        returns {family: ms per call}."""
        check(lib.aocr_profile_enable(self._h, 1), "aocr_profile_enable")
        try:
            tot = np.zeros(len(_lib.PROF_FAMILIES))
            for _ in range(repeats):
                fn()
                ms, marks = (C.c_float * len(_lib.PROF_FAMILIES))(), C.c_int32()
                check(lib.aocr_profile_read(self._h, ms, C.byref(marks)), "aocr_profile_read")
                tot += np.array(list(ms))
        finally:
            check(lib.aocr_profile_enable(self._h, 0), "aocr_profile_enable")
        return {k: float(v / repeats) for k, v in zip(_lib.PROF_FAMILIES, tot)}

    def step(self, batch, forward_only, beam_size=None, trie=None):
        """Returns (loss*batch_size, [num_nonzeros, num_correct]) exactly like model:step (model.lua:695-705)."""
        images, targets, targets_eval = self._upload(batch)
        if trie is not None and trie._dev is None:
            trie.to(self.device)
        num_nonzeros = batch[3]
        B, _, _, W = images.shape
        target_l = targets.shape[1]
        assert target_l <= self.max_decoder_l, f"max_decoder_l ({self.max_decoder_l}) < target_l ({target_l})!"
        check(lib.aocr_model_set_stream(self._h, self._stream()))
        loss_dev = self._scal[0:1]
        if not forward_only:
            global_batch = None
            if dist.world_size() > 1:
                # tail batches differ between ranks (data_gen.lua:123-153): the rows and label counts of the step are summed first, so
                # that d(loss) is scaled by 1 / (global rows) and train.lua:103,120 divides the summed loss by the summed count
                cnt = torch.tensor([float(B), float(num_nonzeros)], dtype=torch.float64, device=self.device)
                torch.distributed.all_reduce(cnt)
                global_batch, num_nonzeros = int(cnt[0].item()), int(cnt[1].item())
            loss_dev = self.train_step_device(images, targets, targets_eval, global_batch)
            loss = float(loss_dev.item())
            self.check_health()
            return loss, [num_nonzeros, 0.0]
        # forward only: beam search + gold pass
        beam_size = beam_size or 1
        beam_size = min(beam_size, self.target_vocab_size)
        Lt = self.max_decoder_l
        labels, scores, gold, loss_dev = self.decode_device(images, targets, targets_eval, beam_size, trie)
        # word scoring on device (evalWordErrRate, utils.lua:136-175): one Levenshtein distance per row, a word is right iff it is 0
        tge_dev = torch.full((B, Lt), PAD, dtype=torch.int32, device=self.device)
        tge_dev[:, :target_l] = targets_eval
        edist, tlen = edit_distance_device(labels, tge_dev, self._stream())
        labels_h = labels.cpu().numpy()
        dist_h, tlen_h = edist.cpu().numpy(), tlen.cpu().numpy()
        word_err = float((dist_h != 0).sum())
        labels_pred, labels_gold = [], []
        if self.visualize:
            _, labels_pred, labels_gold = eval_word_err_rate(labels_h, tge_dev.cpu().numpy(), True)
        accuracy = B - word_err
        self._dec_out = SimpleNamespace(labels=labels_h, scores=scores.cpu().numpy(), gold_scores=gold.cpu().numpy(),
                                        edit_distance=dist_h, target_len=tlen_h)
        if self.visualize and self.visualize_file is not None:
            img_paths = batch[4]
            for i in range(len(img_paths)):                                         # model.lua:628-633
                self.visualize_file.write("%s\t%s\t%s\t%f\t%f\n" % (img_paths[i], labels_gold[i], labels_pred[i],
                                                                    self._dec_out.scores[i], self._dec_out.gold_scores[i]))
            self.visualize_file.flush()
        loss = float(loss_dev.item())
        self.check_health()
        return loss, [num_nonzeros, accuracy]

    def forward_logits(self, batch, training=False):
        """Teacher-forced decoder logits (L,B,V) and NLL sum (parity tap; the pre-LogSoftMax output of output_projector.lua:5)."""
        images, targets, targets_eval = self._upload(batch)
        B, _, _, W = images.shape
        L = targets.shape[1]
        check(lib.aocr_model_set_stream(self._h, self._stream()))
        logits = torch.empty((L, B, self.target_vocab_size), dtype=torch.float32, device=self.device)
        check(lib.aocr_forward_logits(self._h, ptr(images), ptr(targets), ptr(targets_eval), B, W, L, int(training), ptr(logits),
                                      ptr(self._scal[0:1])), "aocr_forward_logits")
        return logits.cpu(), float(self._scal[0].item())

    def train_forward_backward(self, batch, grad_scale=None):
        """feval only (no parameter update): loss sum; gradients stay in self.grad_params."""
        images, targets, targets_eval = self._upload(batch)
        B, _, _, W = images.shape
        L = targets.shape[1]
        check(lib.aocr_model_set_stream(self._h, self._stream()))
        self._arm_dropout()
        check(lib.aocr_train_forward_backward(self._h, ptr(images), ptr(targets), ptr(targets_eval), B, W, L,
                                              (1.0 / B) if grad_scale is None else grad_scale, ptr(self._scal[0:1])),
              "aocr_train_forward_backward")
        return float(self._scal[0].item())

    def cluster_status(self) -> int:
        """0 = healthy; otherwise the code of a whole-sequence kernel that gave up waiting for its group since the last call (read and clear)."""
        code = C.c_int32(0)
        check(lib.aocr_cluster_status(self._h, C.byref(code)), "aocr_cluster_status")
        return int(code.value)

    def check_health(self):
        """Raises if a whole-sequence kernel ever gave up waiting for its group (include/aocr.h: aocr_cluster_status); synchronises."""
        code = C.c_int32(self.cluster_status())
        if code.value != 0:
            raise RuntimeError(f"a cluster kernel timed out waiting for its group (code {code.value}): the results of that step are invalid")

    def _arm_dropout(self):
        """nn.Dropout(p) of LSTM.lua:68-69,116-118 for the coming training step (rank-dependent seed under data parallelism)."""
        if self.dropout > 0.0 or getattr(self, "_dropout_armed", False):
            # mask counter = global_step (train.lua:115 advances it in the host loop) + 2^32 x (training steps already taken at this
            # global_step): a caller that never advances global_step still draws a fresh mask every step, and the first step at a
            # given global_step uses exactly (seed, global_step) -- what the oracle replays (oracle_torch.dropout_state)
            gs = int(self.global_step)
            rep = self._drop_repeat + 1 if gs == self._drop_last_gs else 0
            self._drop_last_gs, self._drop_repeat = gs, rep
            check(lib.aocr_set_dropout(self._h, self.dropout, self.dropout_seed + 7919 * dist.rank(), gs + (rep << 32)), "aocr_set_dropout")
            self._dropout_armed = self.dropout > 0.0

    def sgd_step(self, lr=None, clip=5.0):
        norms = self._scal[2:12]
        check(lib.aocr_sgd_step(self._h, float(self.optim_state["learningRate"] if lr is None else lr), clip, ptr(norms)))
        return norms.cpu().numpy().reshape(5, 2)

    def format_norms(self):
        """the lines optim_sgd.lua:49 prints every step, from the norms the last step() left on the device; reading them is the only
        host sync, so the reference's per-step print becomes an on-demand report."""
        if self.last_norms is None:
            return []
        n = self.last_norms.cpu().numpy().reshape(5, 2)
        return ["i: %d, param norm: %f, grad norm: %f" % (i + 1, n[i, 0], n[i, 1]) for i in range(5)]

    def adadelta_step(self, rho=0.9, eps=1e-6, weight_decay=0.0):
        """optim.adadelta_list (src/optim/optim_adadelta.lua:19-62) on the gradients of the last train_forward_backward; the state
        {paramVariance | accDelta} lives in `self.adadelta_state` (2 x num_params floats on the device)."""
        if getattr(self, "adadelta_state", None) is None:
            self.adadelta_state = torch.zeros(2 * self.num_params, dtype=torch.float32, device=self.device)
        check(lib.aocr_adadelta_step(self._h, rho, eps, weight_decay, ptr(self.adadelta_state)), "aocr_adadelta_step")

    def _adam_alloc(self):
        """`self.adam_state`: aocr_adam_state_bytes zeroed bytes on the device ({m | v | 32-byte tail}, include/aocr.h), 8-byte aligned."""
        nbytes = lib.aocr_adam_state_bytes(self.num_params)
        self._adam_words = torch.zeros(nbytes // 8, dtype=torch.int64, device=self.device)
        self.adam_state = self._adam_words.view(torch.uint8)
        return self.adam_state

    def adam_step(self, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, clip=0.0):
        """AdamW (include/aocr.h: aocr_adam_step) on the gradients of the last train_forward_backward, which it leaves as they are.  The state
        lives in `self.adam_state` (allocated zeroed on first use: a fresh optimizer); the 15 norms {param norm[5], grad norm[5], clip scale[5]}
        stay on the device in `self.last_norms_adam`.  Enqueues only: no host sync."""
        if self.adam_state is None:
            self._adam_alloc()
        if getattr(self, "_adam_norms", None) is None:
            self._adam_norms = torch.zeros(15, dtype=torch.float32, device=self.device)
        p = _lib.AdamParams(lr, betas, eps, weight_decay, clip)
        check(lib.aocr_adam_step(self._h, C.byref(p), ptr(self.adam_state), ptr(self._adam_norms)), "aocr_adam_step")
        self.last_norms_adam = self._adam_norms

    def adam_steps(self) -> int:
        """updates AdamW has applied (the `steps` word of the state's tail; skipped steps do not count).  Synchronises."""
        if self.adam_state is None:
            return 0
        return int(self._adam_words[self.num_params + 2].item())

    # ------------------------------------------------------------------ misc API of the reference class
    def vis(self, output_dir):
        """model:vis, model.lua:708-718."""
        self.visualize = True
        self.visualize_path = os.path.join(output_dir, "results.txt")
        try:
            self.visualize_file = open(self.visualize_path, "w")
        except OSError:
            print(f"Error: visualize file {self.visualize_path} cannot be created")
            self.visualize = False
            self.visualize_file = None

    def save(self, model_path, layout=None):
        """model:save, model.lua:720-725 ({nets, config, global_step, optim_state}).
        layout None: a torch.save file with the flat parameter vector (fast path for this package);  a path ending in .t7 is written
        in Torch7 serialization: layout "flat" (the default for .t7) = one plain Lua table of named FloatTensors (write_flat_checkpoint:
        depends on nothing but torch.load of a table; INTEGRATION.md shows the Lua that pours it into a model the reference has just
        created), layout "reference" (opt-in) = the reference's own table with the five nets as nn / nngraph object trees
        (aocr.checkpoint.write_reference_checkpoint).  The object trees are UNVERIFIED against Torch7 -- nngraph's gModule is an
        nn.Container whose parameters() / type() walk self.modules and whose forward / backward use fg, bg, innode, outnode and
        backwardnodes, none of which can be reproduced faithfully without the un-vendored packages -- so that layout is never what a
        caller gets without asking for it.
        No collective happens here (train.lua saves from one process): under data parallelism WITHOUT synchronised BatchNorm the
        running statistics are rank-local -- every rank calls `sync_bn_state()` before rank 0 saves."""
        if str(model_path).endswith(".t7") or layout in ("reference", "flat"):
            from .checkpoint import write_flat_checkpoint, write_reference_checkpoint
            if layout is None:                                    # the .t7 default is NOT what upstream model:load reads -- say so once per call
                import warnings
                warnings.warn(f"Model.save({str(model_path)!r}): writing the flat 'aocr-flat-1' table; the reference's model:load "
                              "(src/model/model.lua:52-60) reads layout='reference' (or the Lua glue of INTEGRATION.md)", stacklevel=2)
            if self.adam_state is not None and not getattr(self, "_t7_adam_warned", False):
                import warnings
                self._t7_adam_warned = True
                warnings.warn(f"Model.save({str(model_path)!r}): the Torch7 layouts do not carry the AdamW state (adam_state); a run resumed from "
                              "this file restarts its optimizer -- save without .t7 to keep it", stacklevel=2)
            writer = write_reference_checkpoint if layout == "reference" else write_flat_checkpoint
            writer(model_path, {k: v.numpy() for k, v in self.get_parameters().items()},
                   {k: v.numpy() for k, v in self.get_bn_state().items()}, self.config, self.global_step, self.optim_state)
            return
        ck = {"params": self.params.detach().cpu(), "bn_state": self.bn_state.detach().cpu(), "config": self.config,
              "global_step": self.global_step, "optim_state": dict(self.optim_state)}
        if self.adam_state is not None:
            ck["adam_state"] = self.adam_state.detach().cpu()
        torch.save(ck, model_path)

    def sync_bn_state(self):
        """COLLECTIVE (every rank calls it): averages the BatchNorm running statistics over the ranks.  Needed only when the step ran
        with rank-local batch statistics; with synchronised BatchNorm (the default of aocr.dist.attach / attach_rccl) the running
        statistics are already identical on all ranks and this returns without communicating."""
        if dist.world_size() <= 1 or self.sync_bn_active():
            return
        torch.distributed.all_reduce(self.bn_state); self.bn_state.div_(dist.world_size())

    def comm_exposed_ms(self) -> float:
        """ms the model's stream waited for the gradient exchange at the end of the last step (include/aocr.h: aocr_comm_exposed_ms)."""
        ms = C.c_float(0.0)
        check(lib.aocr_comm_exposed_ms(self._h, C.byref(ms)), "aocr_comm_exposed_ms")
        return float(ms.value)

    def sync_bn_active(self) -> bool:
        """True when the library normalises with the statistics of the global batch (asked of the library, include/aocr.h)."""
        n, sb, prov = C.c_int32(), C.c_int32(), C.c_int32()
        check(lib.aocr_comm_info(self._h, C.byref(n), C.byref(sb), C.byref(prov)), "aocr_comm_info")
        return bool(sb.value) and prov.value != 0

    def shutdown(self):
        if self.visualize_file:
            self.visualize_file.close()
            self.visualize_file = None
        if self._h is not None:
            lib.aocr_model_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            if self._h is not None:
                lib.aocr_model_destroy(self._h)
                self._h = None
        except Exception:
            pass
