"""The reference's `Transformer_Autoencoder` (transformer/transformer_model.py:10-175) on the HIP path.

Same constructor signature and the same `state_dict` keys for the encoder (timm 0.3.2 naming: patch_embed.proj.*,
cls_token, pos_embed, blocks.{i}.norm1/attn.qkv/attn.proj/norm2/mlp.fc1/mlp.fc2.*, norm.*), so a checkpoint saved by
`transformer/autoencoder_training.py:128-131` loads with `load_state_dict(..., strict=False)` into the default, encoder-only
module and strictly into `Transformer_Autoencoder(decoder=True)`, which adds decoder_embed, decoder_noise_token,
decoder_pos_embed, decoder_blocks.{i}.*, decoder_norm and decoder_pred and runs forward / forward_decoder / forward_loss /
reconstruct through `os_vit_decode` (transformer/autoencoder_load.py:57-67).  `forward_encoder(x)` takes (N,1,224,224) in [0,1]
(gru/gru_test.py:49-53) and returns (N,1,128) like the reference; it runs `os_vit_encode` (hand-written HIP kernels only: fp32-MFMA GEMM with fused epilogues, MFMA attention).
Parity: the reference's own class (unmodified glue: patch + position table, cls token, block loop, final LayerNorm, token 0, sigmoid)
around a plain-torch restatement of the timm-0.3.2 blocks (golden G11) and around Hugging Face transformers' ViTLayer (G14: identical
float32 latents); timm 0.3.2 itself and the trained weights are absent from the image.
"""
import ctypes as C

import numpy as np
import torch
import torch.nn as nn

from . import _capi
from .engine import default_engine, _ptr


def _sincos_pos_embed(dim, grid):
    def one_d(d, pos):
        omega = 1.0 / 10000 ** (np.arange(d // 2, dtype=np.float64) / (d / 2.0))
        out = np.einsum("m,d->md", pos.reshape(-1), omega)
        return np.concatenate([np.sin(out), np.cos(out)], axis=1)
    gh, gw = np.arange(grid, dtype=np.float32), np.arange(grid, dtype=np.float32)
    g = np.stack(np.meshgrid(gw, gh), axis=0).reshape(2, 1, grid, grid)          # w first (pos_embed.py:27)
    emb = np.concatenate([one_d(dim // 2, g[0]), one_d(dim // 2, g[1])], axis=1)
    return np.concatenate([np.zeros((1, dim)), emb], axis=0)


class _Attn(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.qkv = nn.Linear(dim, dim * 3, bias=True)
        self.proj = nn.Linear(dim, dim)


class _Mlp(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.fc2 = nn.Linear(hidden, dim)


class _Block(nn.Module):          # weight container with timm's parameter names
    def __init__(self, dim, hidden):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim)
        self.attn = _Attn(dim)
        self.norm2 = nn.LayerNorm(dim)
        self.mlp = _Mlp(dim, hidden)


class _PatchEmbed(nn.Module):
    def __init__(self, img_size, patch_size, in_chans, embed_dim):
        super().__init__()
        self.patch_size = (patch_size, patch_size)
        self.num_patches = (img_size // patch_size) ** 2
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=patch_size, stride=patch_size)


_BLOCK_KEYS = ("norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias",
               "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")


class _VitTrainFn(torch.autograd.Function):
    # Every forward owns its saved activations (a workspace tensor kept in the autograd ctx) and pins the flat weights it ran
    # with, so any number of graphs may be alive at once (m(a)[0] + m(b)[0], gradient accumulation, another module's call in
    # between: the engine's scratch and its loaded weights are shared per device).  pred is marked non-differentiable.
    @staticmethod
    def forward(ctx, imgs, module, *params):
        eng = module._engine(imgs)
        img = module._frames(imgs.detach())
        N, dev = img.shape[0], img.device
        with eng.lock:                                     # load + forward as one unit: a context holds ONE auto-encoder
            module._load_locked(eng, dev)
            _, flat, dflat = module._loaded
            nws = eng.lib.os_vit_train_ws_floats(eng._h, N)
            if nws == 0:
                raise RuntimeError(f"os_vit_train_ws_floats: {eng.lib.os_last_error(eng._h).decode()}")
            ws = torch.empty(nws, dtype=torch.float32, device=dev)
            pred = torch.empty((N, module.num_patches, module.patch_size ** 2 * module.in_chans), dtype=torch.float32, device=dev)
            loss = torch.empty((), dtype=torch.float32, device=dev)
            eng._check(eng.lib.os_vit_forward_train(eng._h, N, _ptr(img), _ptr(ws), _ptr(pred), _ptr(loss), eng._stream()),
                       "os_vit_forward_train")
        ctx.module, ctx.eng = module, eng                 # backward runs on autograd's thread: the SAME context, not that thread's
        ctx.save_for_backward(img, ws, flat, dflat)
        ctx.mark_non_differentiable(pred)
        return loss, pred

    @staticmethod
    def backward(ctx, dloss, _dpred):
        img, ws, flat, dflat = ctx.saved_tensors
        module, eng = ctx.module, ctx.eng
        genc, gdec = torch.empty_like(flat), torch.empty_like(dflat)
        with eng.lock:
            module._load_flats_locked(eng, flat, dflat)    # the weights this forward ran with (usually still the loaded ones)
            eng._check(eng.lib.os_vit_backward(eng._h, img.shape[0], _ptr(img), _ptr(ws), _ptr(dloss.to(torch.float32).contiguous()),
                                               _ptr(genc), _ptr(gdec), eng._stream()), "os_vit_backward")
        grads = []
        for p, (which, off) in zip(module._train_params(), module._train_offsets()):
            grads.append((genc if which == 0 else gdec)[off:off + p.numel()].view_as(p) if p.requires_grad else None)
        return (None, None, *grads)


class Transformer_Autoencoder(nn.Module):
    """The reference's constructor arguments, then `decoder`.  With decoder=False (default) the module is the encoder alone:
    encoder keys only, and forward() raises NotImplementedError.  With decoder=True it also owns the reference's decoder_*
    parameters under the reference's names (a reference checkpoint loads strictly) and forward / forward_decoder / forward_loss /
    patchify / unpatchify return what the reference's return; reconstruct(imgs) is unpatchify(forward(imgs)[1]) in one call.
    A context holds ONE auto-encoder: another module's call on the same engine evicts this one's weights.
    With decoder=True and trainable=True, forward(imgs) under enabled gradients returns a loss with a grad_fn: the reference's
    training loop (transformer/autoencoder_training.py:103-114: loss.backward(), torch.optim.AdamW.step()) runs on the HIP forward
    and backward (os_vit_forward_train / os_vit_backward); torch supplies memory, the autograd bookkeeping and the optimiser.
    pos_embed and decoder_pos_embed stay fixed as in the reference, and pred is NOT differentiable (marked so): only the loss
    carries the graph.  Under torch.no_grad() a trainable module takes the inference path."""

    def __init__(self, img_size=224, patch_size=16, in_chans=1, embed_dim=128, depth=3, num_heads=4,
                 decoder_embed_dim=128, decoder_depth=3, decoder_num_heads=4, mlp_ratio=4., norm_layer=nn.LayerNorm,
                 decoder=False, trainable=False):
        super().__init__()
        if trainable and not decoder:
            raise ValueError("Transformer_Autoencoder(trainable=True) needs decoder=True: the loss is the decoder's")
        self.trainable = bool(trainable)
        self.in_chans, self.img_size, self.patch_size = in_chans, img_size, patch_size
        self.embed_dim, self.depth, self.num_heads = embed_dim, depth, num_heads
        self.mlp_hidden = int(embed_dim * mlp_ratio)
        self.patch_embed = _PatchEmbed(img_size, patch_size, in_chans, embed_dim)
        self.num_patches = self.patch_embed.num_patches
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, self.num_patches + 1, embed_dim), requires_grad=False)
        self.blocks = nn.ModuleList([_Block(embed_dim, self.mlp_hidden) for _ in range(depth)])
        self.norm = nn.LayerNorm(embed_dim)
        grid = int(self.num_patches ** .5)
        self.pos_embed.data.copy_(torch.from_numpy(_sincos_pos_embed(embed_dim, grid)).float().unsqueeze(0))
        self.has_decoder = bool(decoder)
        if self.has_decoder:                                           # transformer_model.py:36-47
            self.decoder_embed_dim, self.decoder_depth, self.decoder_num_heads = decoder_embed_dim, decoder_depth, decoder_num_heads
            self.decoder_mlp_hidden = int(decoder_embed_dim * mlp_ratio)
            self.decoder_embed = nn.Linear(embed_dim, decoder_embed_dim, bias=True)
            self.decoder_noise_token = nn.Parameter(torch.zeros(1, 1, decoder_embed_dim))
            self.decoder_pos_embed = nn.Parameter(torch.zeros(1, self.num_patches + 1, decoder_embed_dim), requires_grad=False)
            self.decoder_blocks = nn.ModuleList([_Block(decoder_embed_dim, self.decoder_mlp_hidden) for _ in range(decoder_depth)])
            self.decoder_norm = nn.LayerNorm(decoder_embed_dim)
            self.decoder_pred = nn.Linear(decoder_embed_dim, patch_size ** 2 * in_chans, bias=True)
            self.decoder_pos_embed.data.copy_(torch.from_numpy(_sincos_pos_embed(decoder_embed_dim, grid)).float().unsqueeze(0))
            torch.nn.init.normal_(self.decoder_noise_token, std=.02)   # transformer_model.py:69
        torch.nn.init.normal_(self.cls_token, std=.02)                 # transformer_model.py:66
        w = self.patch_embed.proj.weight.data
        torch.nn.init.xavier_uniform_(w.view([w.shape[0], -1]))        # transformer_model.py:62-63
        for m in self.modules():                                       # transformer_model.py:71-82
            if isinstance(m, nn.Linear):
                torch.nn.init.xavier_uniform_(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
        self._loaded = None
        self._adopted = None       # (encoder, decoder) flat vectors of a VitTrainer: the parameters are views of them

    def _adopted_flats(self):
        """The trainer's vectors while the parameters still are views of them; model.to(...), load_state_dict(assign=True) and
        the like rebind the parameters, and the adoption ends there: the module concatenates again (its trainer's next step then
        fails with -5, its vectors no longer being the loaded ones)."""
        a = self._adopted
        if a is not None and any(p.data_ptr() != a[which].data_ptr() + 4 * off
                                 for p, (which, off) in zip(self._train_params(), self._train_offsets())):
            a = self._adopted = None
        return a

    def _flat(self, dev):
        if self._adopted_flats() is not None:
            return self._adopted[0]
        sd = self.state_dict()
        parts = [sd["patch_embed.proj.weight"].reshape(-1), sd["patch_embed.proj.bias"], sd["cls_token"].reshape(-1),
                 sd["pos_embed"].reshape(-1)]
        for i in range(self.depth):
            parts += [sd[f"blocks.{i}.{k}"].reshape(-1) for k in _BLOCK_KEYS]
        parts += [sd["norm.weight"], sd["norm.bias"]]
        return torch.cat([t.detach().float().reshape(-1) for t in parts]).to(dev).contiguous()

    def _flat_decoder(self, dev):
        """include/optistate_hip.h (os_vit_load_decoder): the decoder's flat weight vector."""
        if self._adopted_flats() is not None:
            return self._adopted[1]
        sd = self.state_dict()
        parts = [sd["decoder_embed.weight"], sd["decoder_embed.bias"], sd["decoder_noise_token"], sd["decoder_pos_embed"]]
        for i in range(self.decoder_depth):
            parts += [sd[f"decoder_blocks.{i}.{k}"] for k in _BLOCK_KEYS]
        parts += [sd["decoder_norm.weight"], sd["decoder_norm.bias"], sd["decoder_pred.weight"], sd["decoder_pred.bias"]]
        return torch.cat([t.detach().float().reshape(-1) for t in parts]).to(dev).contiguous()

    def _train_params(self):
        """Parameters in the order of the two flat layouts (_flat, then _flat_decoder)."""
        ps = [self.patch_embed.proj.weight, self.patch_embed.proj.bias, self.cls_token, self.pos_embed]
        for blocks in (self.blocks, self.decoder_blocks):
            for b in blocks:
                ps += [b.norm1.weight, b.norm1.bias, b.attn.qkv.weight, b.attn.qkv.bias, b.attn.proj.weight, b.attn.proj.bias,
                       b.norm2.weight, b.norm2.bias, b.mlp.fc1.weight, b.mlp.fc1.bias, b.mlp.fc2.weight, b.mlp.fc2.bias]
            if blocks is self.blocks:
                ps += [self.norm.weight, self.norm.bias, self.decoder_embed.weight, self.decoder_embed.bias, self.decoder_noise_token,
                       self.decoder_pos_embed]
        return ps + [self.decoder_norm.weight, self.decoder_norm.bias, self.decoder_pred.weight, self.decoder_pred.bias]

    def _train_offsets(self):
        """(0 = encoder vector | 1 = decoder vector, offset) of every _train_params() entry."""
        out, which, off = [], 0, 0
        for p in self._train_params():
            if p is self.decoder_embed.weight:
                which, off = 1, 0
            out.append((which, off))
            off += p.numel()
        return out

    def _decoder_dims(self):
        return _capi.OsVitDims(self.img_size, self.patch_size, self.in_chans, self.decoder_embed_dim, self.decoder_depth,
                               self.decoder_num_heads, self.decoder_mlp_hidden)

    def _engine(self, t):
        if not t.is_cuda:
            raise RuntimeError("optistate_amd Transformer_Autoencoder needs a tensor on the MI355X (no CPU fallback)")
        return default_engine(t.device.index or 0)         # the calling thread's context on this GPU

    def forward_encoder(self, x):
        if not x.is_cuda:
            raise RuntimeError("optistate_amd Transformer_Autoencoder.forward_encoder needs a tensor on the MI355X (no CPU fallback)")
        eng = default_engine(x.device.index or 0)          # the calling thread's context on this GPU
        with eng.lock:                                     # load + encode as one unit: a context holds ONE auto-encoder
            return self._encode_locked(eng, x)

    def preprocess(self, frames, augment=None):
        """uint8 frames (N,H,W,3) | (N,H,W,1) | (N,H,W) on the device (or a numpy array) -> (N,1,img_size,img_size) float32: the
        reference's `transform(img).unsqueeze(0)` (gru/gru_test.py:49-53,122-124), batched, bit for bit (Engine.ingest_frames).
        augment: float64 (N,20) records (optistate_amd.augment.sample_params) -> the training transform of
        transformer/autoencoder_training.py:42-53 instead, the random augmentations between Grayscale and ToTensor applied with these
        parameters (Engine.ingest_frames_u8 + Engine.augment_frames); img_size <= 256."""
        eng = default_engine(frames.device.index or 0) if torch.is_tensor(frames) and frames.is_cuda else default_engine(0)
        if augment is not None:
            return eng.augment_frames(eng.ingest_frames_u8(frames, self.img_size), augment).unsqueeze(1)
        return eng.ingest_frames(frames, self.img_size).unsqueeze(1)

    def encode_frames(self, frames):
        """forward_encoder(preprocess(frames)) in one call (os_vit_encode_frames): (N,1,embed_dim), the same bits."""
        eng = default_engine(frames.device.index or 0) if torch.is_tensor(frames) and frames.is_cuda else default_engine(0)
        fr, N, H, W, Cn = eng._frames_u8(frames)
        with eng.lock:                                     # load + encode as one unit: a context holds ONE auto-encoder
            self._load_locked(eng, fr.device)
            lat = torch.empty((N, self.embed_dim), dtype=torch.float32, device=fr.device)
            eng._check(eng.lib.os_vit_encode_frames(eng._h, N, C.c_void_p(fr.data_ptr()), H, W, Cn, _ptr(lat), eng._stream()),
                       "os_vit_encode_frames")
        return lat.reshape(N, 1, self.embed_dim)

    def _load_locked(self, eng, dev):
        versions = tuple((p.data_ptr(), p._version) for p in self.parameters())
        if self._loaded is not None and self._loaded[0] == versions and getattr(eng, "_vit_owner", None) is self:
            return
        if self._adopted_flats() is not None:
            self._loaded = None    # the same vectors with other contents (a write through torch): pack them again
        self._load_flats_locked(eng, self._flat(dev), self._flat_decoder(dev) if self.has_decoder else None, versions)

    def _load_flats_locked(self, eng, flat, dflat, versions=None):
        """Loads these flat vectors unless they are the loaded ones (versions None: a backward's pinned weights, which the next
        forward must not mistake for the parameters' current values)."""
        if self._loaded is not None and self._loaded[1] is flat and self._loaded[2] is dflat and getattr(eng, "_vit_owner", None) is self:
            return
        d = _capi.OsVitDims(self.img_size, self.patch_size, self.in_chans, self.embed_dim, self.depth, self.num_heads,
                            self.mlp_hidden)
        assert flat.numel() == eng.lib.os_vit_param_count(C.byref(d)), "flat ViT weight vector has the wrong length"
        eng._check(eng.lib.os_vit_load(eng._h, C.byref(d), _ptr(flat)), "os_vit_load")
        if self.has_decoder:
            dd = self._decoder_dims()
            assert dflat.numel() == eng.lib.os_vit_decoder_param_count(C.byref(dd), self.embed_dim), \
                "flat ViT decoder weight vector has the wrong length"
            eng._check(eng.lib.os_vit_load_decoder(eng._h, C.byref(dd), self.embed_dim, _ptr(dflat)), "os_vit_load_decoder")
        self._loaded = (versions, flat, dflat)     # keep the flat tensors alive: the library references them
        eng._vit_owner = self                      # a context holds ONE auto-encoder: another module's load evicts this one

    def _encode_locked(self, eng, x):
        self._load_locked(eng, x.device)
        N = x.shape[0]
        img = x.reshape(N, self.img_size, self.img_size).to(torch.float32).contiguous()
        lat = torch.empty((N, self.embed_dim), dtype=torch.float32, device=x.device)
        eng._check(eng.lib.os_vit_encode(eng._h, N, _ptr(img), _ptr(lat), eng._stream()), "os_vit_encode")
        return lat.reshape(N, 1, self.embed_dim)

    def _need_decoder(self):
        if not self.has_decoder:
            raise NotImplementedError("only forward_encoder (the latent used by the GRU, gru/gru_test.py:119-132) is implemented; "
                                      "the decoder and reconstruction loss need Transformer_Autoencoder(..., decoder=True)")

    def _decode_locked(self, eng, latent, img, want_pred, want_recon, want_loss):
        """One os_vit_decode: latent (N,1,D) -> (pred | None, recon | None, loss | None)."""
        self._load_locked(eng, latent.device)
        N, dev = latent.shape[0], latent.device
        lat = latent.reshape(N, self.embed_dim).to(torch.float32).contiguous()
        pred = torch.empty((N, self.num_patches, self.patch_size ** 2 * self.in_chans), dtype=torch.float32, device=dev) if want_pred else None
        recon = torch.empty((N, self.in_chans, self.img_size, self.img_size), dtype=torch.float32, device=dev) if want_recon else None
        loss = torch.empty((), dtype=torch.float32, device=dev) if want_loss else None
        eng._check(eng.lib.os_vit_decode(eng._h, N, _ptr(lat), _ptr(img) if want_loss else None, _ptr(pred), _ptr(recon), _ptr(loss),
                                         eng._stream()), "os_vit_decode")
        return pred, recon, loss

    def _frames(self, imgs):
        return imgs.reshape(imgs.shape[0], self.img_size, self.img_size).to(torch.float32).contiguous()

    def forward_decoder(self, x):
        """latent (N,1,embed_dim) -> pred (N, num_patches, patch_size**2 * in_chans)   (transformer_model.py:137-159)"""
        self._need_decoder()
        eng = self._engine(x)
        with eng.lock:
            return self._decode_locked(eng, x, None, True, False, False)[0]

    def forward_loss(self, imgs, pred):
        """mean((patchify(imgs) - pred)**2) as a 0-d device tensor   (transformer_model.py:161-169)"""
        self._need_decoder()
        eng = self._engine(pred)
        with eng.lock:
            self._load_locked(eng, pred.device)
            loss = torch.empty((), dtype=torch.float32, device=pred.device)
            eng._check(eng.lib.os_vit_recon_loss(eng._h, pred.shape[0], _ptr(self._frames(imgs)), _ptr(pred.to(torch.float32).contiguous()),
                                                 _ptr(loss), eng._stream()), "os_vit_recon_loss")
        return loss

    def forward(self, imgs):
        """(loss, pred) like the reference (transformer_model.py:171-175): os_vit_encode + one os_vit_decode; in a trainable
        module under enabled gradients os_vit_forward_train, with loss.backward() on os_vit_backward (pred: no gradient)."""
        self._need_decoder()
        eng = self._engine(imgs)
        if self.trainable and torch.is_grad_enabled():
            return _VitTrainFn.apply(imgs, self, *self._train_params())
        with eng.lock:
            lat = self._encode_locked(eng, imgs)
            pred, _, loss = self._decode_locked(eng, lat, self._frames(imgs), True, False, True)
        return loss, pred

    def reconstruct(self, imgs):
        """imgs (N,1,H,W) -> the decoder's image (N,1,H,W) = unpatchify(forward(imgs)[1]), written by the decoder's last kernel."""
        self._need_decoder()
        eng = self._engine(imgs)
        with eng.lock:
            lat = self._encode_locked(eng, imgs)
            return self._decode_locked(eng, lat, None, False, True, False)[1]

    def patchify(self, imgs):
        """(N, in_chans, H, W) -> (N, L, patch_size**2 * in_chans)   (transformer_model.py:84-96)"""
        p = self.patch_size
        assert imgs.shape[2] == imgs.shape[3] and imgs.shape[2] % p == 0
        h = w = imgs.shape[2] // p
        x = imgs.reshape(imgs.shape[0], self.in_chans, h, p, w, p)
        return torch.einsum("nchpwq->nhwpqc", x).reshape(imgs.shape[0], h * w, p ** 2 * self.in_chans)

    def unpatchify(self, x):
        """(N, L, patch_size**2 * in_chans) -> (N, in_chans, H, W)   (transformer_model.py:98-110)"""
        p = self.patch_size
        h = w = int(x.shape[1] ** .5)
        assert h * w == x.shape[1]
        x = x.reshape(x.shape[0], h, w, p, p, self.in_chans)
        return torch.einsum("nhwpqc->nchpwq", x).reshape(x.shape[0], self.in_chans, h * p, h * p)
