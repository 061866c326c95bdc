"""Full fine-tuning engines: ``disable_lora: true`` of the reference (bioscanclip/model/simple_clip.py:125-203,
config/model_config/full_fine_tuning/**) -- every parameter of the towers is trained (:199-201), the BERT encoders carry no
LoRA branch and the ViT keeps LoRA on all blocks (the reference's own quirk: an empty ``lora_layer`` list is falsy in
image_encoder.py:56-59 and means "all layers").

This file holds the FT parameter layout, the per-step repacking of the operands and the gradient hooks; the kernel sequences,
forward and backward, are the LoRA-regime engines' own (hip/engine.py).  The forward re-packs the bf16 operand copies of the
weights from the f32 masters every step and keeps the inputs of fc1 / fc2 per layer.  The backward calls the hooks below for the
gradients the LoRA regime never needs:
  * ``_dw``, in front of every dX GEMM -- Linear weights: dW = dY^T X on the same MFMA GEMM with both operands transposed (as the
    trainable heads always did), accumulated in f32 into the flat gradient buffer; biases by ``bsclip_colsum``;
  * ``_ln_dw``, in front of every LayerNorm backward -- gains / biases (``bsclip_ln_param_grad``);
  * ``_below_layer0`` -- the dX chain continues through layer 0 into the embeddings: BertEmbeddings tables
    (``bsclip_embed_grad``), ViT patch filters (``bsclip_gather_cast_rows`` + the dW GEMM), cls token and position table
    (ordered column sums).
All trainable tensors live in one flat f32 buffer per engine; q / k / v weights (and biases) of a BERT layer are adjacent in
it, so the fused [3H, H] operand and its gradient are plain views.
"""
import torch

from . import ops
from .engine import BF16, F32, BertEngine, ViTEngine, split_plan, tok0
from .lib import EPI_RESID_F32


class _FTMixin:
    _partial = None

    # ------------------------------------------------------------------------------------------------ flat-buffer access
    def tp(self, name, shape=None, n=None, grad=False):
        """View of trunk tensor ``name`` (or of ``n`` elements starting at it) in the flat data / gradient buffer."""
        i = self._trunk_index + self._t[name]
        if shape is None and n is None:
            shape = self.flat.params[i].shape
        return self.flat.view(i, shape, n=n, grad=grad)

    def _register(self, named):
        self._t = {name: i for i, (name, _) in enumerate(named)}
        return [p for _, p in named]

    # --------------------------------------------------------------------------------------------- weight re-packing
    def _repack(self):
        """bf16 operand copies (and their transposes for the dX GEMMs) from the f32 masters; once per forward."""
        for w32, dst, dst_t, aug in self._packs:
            if aug is None:
                ops.cast_f32_bf16(w32, dst)
                if dst_t is not None:
                    ops.transpose_bf16(dst, dst.shape[0], dst.shape[1], dst_t)
            else:  # fused QKV: the forward operand is the [3H, H + KPAD] K-augmented matrix
                ops.cast_f32_bf16(w32, self._wtmp[: w32.shape[0]])
                ops.transpose_bf16(self._wtmp[: w32.shape[0]], w32.shape[0], w32.shape[1], dst_t)
                ops.transpose_bf16(dst_t, w32.shape[1], w32.shape[0], aug)

    def refresh_lora_weights(self):
        self._repack()
        super().refresh_lora_weights()

    # ------------------------------------------------------------------------------------------------ weight gradients
    def _tbuf(self, tag, rows, M, Mp):
        """Zero-padded transposed operand [rows, Mp] of a weight-gradient GEMM over M tokens.  Keyed by M as well: the columns
        [M, Mp) must stay zero, and two GEMMs with different token counts (the ViT blocks' B * 197 and the patch embedding's
        B * 196 round to the same Mp) would otherwise leave each other's last columns behind."""
        key = (tag, rows, M, Mp)
        b = self._tbufs.get(key)
        if b is None:
            b = self._tbufs[key] = torch.zeros(rows, Mp, dtype=BF16, device=self.device)
        return b

    def _dw(self, dY, X, M, N, K, wname, bname, w_n=None):
        """grad(W[N,K]) += dY[:M,:N]^T X[:M,:K];  grad(b[N]) += column sums of dY."""
        S, Mp = split_plan(M, N, K)
        tA, tB = self._tbuf("A", N, M, Mp), self._tbuf("B", K, M, Mp)
        if bname is not None:   # the bias gradient falls out of the transpose's tiles
            ops.transpose_colsum_bf16(dY, M, N, tA, self.tp(bname, n=N if w_n is not None else None, grad=True))
        else:
            ops.transpose_bf16(dY, M, N, tA)
        ops.transpose_bf16(X, M, K, tB)
        gW = self.tp(wname, (N, K), n=w_n, grad=True)
        if S > 1:
            if self._partial is None:
                self._partial = torch.empty(512 * 65536, dtype=F32, device=self.device)   # splits * tiles <= 512 slabs of 256 x 256
            ops.gemm_splitk_f32(tA, tB, gW, S, self._partial, K=Mp)
        else:
            ops.gemm(tA, tB, gW, EPI_RESID_F32, resid=gW, K=Mp)

    def _ln_dw(self, x, stats, mode, wname, bname, **grads):
        """grad(gain), grad(bias) += ...; ``grads``: those of the following layernorm_bwd's g_resid / g_gemm / dt / lora_a / in_dropout
        that pass through the normalisation (a pre-LN block's g_resid does not)."""
        ops.ln_param_grad(x, stats, mode, self.tp(wname, grad=True), self.tp(bname, grad=True), **grads)


# ============================================================================================================== ViT
class ViTEngineFT(_FTMixin, ViTEngine):
    def __init__(self, module, device, mode, reuse_flat=None):
        assert mode.full_ft
        self._module = module
        self._tbufs = {}
        super().__init__(module, device, mode, reuse_flat)
        vit = module.lora_vit
        H = self.H
        # live f32 views (the parameters were re-homed into the flat buffer by the base constructor)
        self.cls = vit.cls_token.data.view(-1)
        self.pos = vit.pos_embed.data.view(self.S, H)
        self.b_patch = vit.patch_embed.proj.bias.data
        self.ln_f = (vit.norm.weight.data, vit.norm.bias.data)
        self._wtmp = torch.empty(3 * H, H, dtype=BF16, device=device)
        self._packs = [(vit.patch_embed.proj.weight.data.view(H, -1), self.w_patch, None, None)]
        for blk, lay in zip(vit.blocks, self.layers):
            q = blk.attn.qkv
            base = q.qkv if hasattr(q, "linear_a_q") else q
            lay.b_qkv = base.bias.data
            lay.ln1 = (blk.norm1.weight.data, blk.norm1.bias.data)
            lay.ln2 = (blk.norm2.weight.data, blk.norm2.bias.data)
            lay.b_proj, lay.b_fc1, lay.b_fc2 = blk.attn.proj.bias.data, blk.mlp.fc1.bias.data, blk.mlp.fc2.bias.data
            self._packs += [(base.weight.data, None, lay.wqkv_t, lay.waug[:, :H]),
                            (blk.attn.proj.weight.data, lay.w_proj, lay.w_proj_t, None),
                            (blk.mlp.fc1.weight.data, lay.w_fc1, lay.w_fc1_t, None),
                            (blk.mlp.fc2.weight.data, lay.w_fc2, lay.w_fc2_t, None)]

    def _trunk_trainables(self):
        vit = self._module.lora_vit
        named = [("cls", vit.cls_token), ("pos", vit.pos_embed), ("patch.w", vit.patch_embed.proj.weight),
                 ("patch.b", vit.patch_embed.proj.bias)]
        for i, blk in enumerate(vit.blocks):
            q = blk.attn.qkv
            base = q.qkv if hasattr(q, "linear_a_q") else q
            named += [(f"{i}.n1.w", blk.norm1.weight), (f"{i}.n1.b", blk.norm1.bias), (f"{i}.qkv.w", base.weight),
                      (f"{i}.qkv.b", base.bias), (f"{i}.proj.w", blk.attn.proj.weight), (f"{i}.proj.b", blk.attn.proj.bias),
                      (f"{i}.n2.w", blk.norm2.weight), (f"{i}.n2.b", blk.norm2.bias), (f"{i}.fc1.w", blk.mlp.fc1.weight),
                      (f"{i}.fc1.b", blk.mlp.fc1.bias), (f"{i}.fc2.w", blk.mlp.fc2.weight), (f"{i}.fc2.b", blk.mlp.fc2.bias)]
        named += [("norm.w", vit.norm.weight), ("norm.b", vit.norm.bias)]
        return self._register(named)

    def _extend_workspace(self, ws):
        ws["dyp"] = torch.empty(ws["B"] * 196, self.H, dtype=BF16, device=self.device)   # patch rows of d x0, bf16

    def _below_layer0(self, ws):
        """d x0 [B, 197, H]: x0[b, 0] = cls + pos[0], x0[b, 1 + p] = patch_p W^T + b + pos[1 + p]."""
        B, S, H, dx = ws["B"], self.S, self.H, ws["dx"]
        ops.colsum(dx.view(B, S * H), B, S * H, self.tp("pos", grad=True).view(-1))      # ordered sum over the batch
        ops.colsum(tok0(dx, B), B, H, self.tp("cls", grad=True).view(-1))
        ops.gather_cast_rows(dx, B * 196, S, 196, 1, ws["dyp"])
        self._dw(ws["dyp"], ws["cols"], B * 196, H, ws["cols"].shape[1], "patch.w", "patch.b")


# ============================================================================================================= BERT
class BertEngineFT(_FTMixin, BertEngine):
    def __init__(self, module_bert, head, head_modules, device, mode, reuse_flat=None):
        assert mode.full_ft
        self._module = module_bert
        self._head_modules = head_modules
        self._head_kind = head
        self._tbufs = {}
        super().__init__(module_bert, head, head_modules, device, mode, reuse_flat)
        bert, H = module_bert, self.H
        emb = bert.embeddings
        self.word, self.posw = emb.word_embeddings.weight.data, emb.position_embeddings.weight.data
        self.typew = emb.token_type_embeddings.weight.data
        self.ln_e = (emb.LayerNorm.weight.data, emb.LayerNorm.bias.data)
        pid = getattr(emb.word_embeddings, "padding_idx", None)    # HF: padding_idx = config.pad_token_id = 0
        self.pad_id = -1 if pid is None else int(pid)
        self._wtmp = torch.empty(3 * H, H, dtype=BF16, device=device)
        self._packs = []
        for i, (layer, lay) in enumerate(zip(bert.encoder.layer, self.layers)):
            lay.b_qkv = self.tp(f"{i}.q.b", n=3 * H)
            lay.b_o = layer.attention.output.dense.bias.data
            lay.ln_a = (layer.attention.output.LayerNorm.weight.data, layer.attention.output.LayerNorm.bias.data)
            lay.b_fc1, lay.b_fc2 = layer.intermediate.dense.bias.data, layer.output.dense.bias.data
            lay.ln_b = (layer.output.LayerNorm.weight.data, layer.output.LayerNorm.bias.data)
            self._packs += [(self.tp(f"{i}.q.w", (3 * H, H), n=3 * H * H), None, lay.wqkv_t, lay.waug[:, :H]),
                            (layer.attention.output.dense.weight.data, lay.w_o, lay.w_o_t, None),
                            (layer.intermediate.dense.weight.data, lay.w_fc1, lay.w_fc1_t, None),
                            (layer.output.dense.weight.data, lay.w_fc2, lay.w_fc2_t, None)]
        if head == "mlm_softmax_mean":
            tr = head_modules[0]
            self.b_tr = tr.dense.bias.data
            self.ln_t = (tr.LayerNorm.weight.data, tr.LayerNorm.bias.data)
            self._packs.append((tr.dense.weight.data, self.w_tr, self.w_tr_t, None))

    def _trunk_trainables(self):
        bert = self._module
        emb = bert.embeddings
        named = [("word", emb.word_embeddings.weight), ("posw", emb.position_embeddings.weight),
                 ("typew", emb.token_type_embeddings.weight), ("lne.w", emb.LayerNorm.weight), ("lne.b", emb.LayerNorm.bias)]
        for i, layer in enumerate(bert.encoder.layer):
            sa = layer.attention.self
            lin = lambda m: m.w if hasattr(m, "w_a") else m
            q, k, v = lin(sa.query), lin(sa.key), lin(sa.value)
            # q / k / v adjacent: the fused [3H, H] operand, its bias and both gradients are plain views of the flat buffers
            named += [(f"{i}.q.w", q.weight), (f"{i}.k.w", k.weight), (f"{i}.v.w", v.weight), (f"{i}.q.b", q.bias),
                      (f"{i}.k.b", k.bias), (f"{i}.v.b", v.bias), (f"{i}.o.w", layer.attention.output.dense.weight),
                      (f"{i}.o.b", layer.attention.output.dense.bias), (f"{i}.lna.w", layer.attention.output.LayerNorm.weight),
                      (f"{i}.lna.b", layer.attention.output.LayerNorm.bias), (f"{i}.fc1.w", layer.intermediate.dense.weight),
                      (f"{i}.fc1.b", layer.intermediate.dense.bias), (f"{i}.fc2.w", layer.output.dense.weight),
                      (f"{i}.fc2.b", layer.output.dense.bias), (f"{i}.lnb.w", layer.output.LayerNorm.weight),
                      (f"{i}.lnb.b", layer.output.LayerNorm.bias)]
        if self._head_kind == "mlm_softmax_mean":
            tr = self._head_modules[0]
            named += [("tr.w", tr.dense.weight), ("tr.b", tr.dense.bias), ("lnt.w", tr.LayerNorm.weight), ("lnt.b", tr.LayerNorm.bias)]
        return self._register(named)

    def _extend_workspace(self, ws):
        ws["demb"] = torch.empty(ws["M"], self.H, dtype=F32, device=self.device)

    def _below_layer0(self, ws, g_resid, g_gemm, dt_in, a_in):
        """The embedding LayerNorm (its output was dropped in forward with site (-1, 0)) and the three tables."""
        e_drop = self._drop(ws, self.p_hidden, -1, 0)
        self._ln_dw(ws["emb"], ws["st_e"], 1, "lne.w", "lne.b", g_resid=g_resid, g_gemm=g_gemm, dt=dt_in, lora_a=a_in,
                    in_dropout=e_drop)
        ops.layernorm_bwd(ws["emb"], ws["st_e"], self.ln_e[0], 1, g_resid=g_resid, g_gemm=g_gemm, dt=dt_in, lora_a=a_in,
                          dx_f32=ws["demb"], in_dropout=e_drop)
        ids = ws["ids"].contiguous()
        tt = ws["type_ids"]
        ops.embed_grad(ids, None if tt is None else tt.contiguous(), ws["demb"], self.tp("word", grad=True),
                       self.tp("posw", grad=True), self.tp("typew", grad=True), pad_id=self.pad_id)
