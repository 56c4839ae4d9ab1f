"""SD UNet forward executed entirely by the HIP kernels of libfreefine_hip.so (no torch math on the path).

Replaces: override_forward.forward (/root/reference/src/utils/attention.py:11-225) + the diffusers-0.18 blocks it
drives + the hooked Attention.forward (attention.py:350-418), returning a bare [B,4,h,w] fp32 tensor like the reference.

MI355X-first layout decisions
  * activations are [B, H*W, C] (channel-contiguous) end to end: conv (implicit GEMM), GroupNorm, LayerNorm, attention and
    the Linear layers all read/write the same buffers -- the NCHW<->NLC transposes of the reference do not exist;
  * every weight is repacked once to [N][Kpad] (K contiguous); conv weights to (ky,kx,ci) order; GEGLU projections are
    interleaved so hidden*gelu(gate) happens in the GEMM epilogue; the 22 time-embedding projections are one GEMM;
  * V is produced transposed by its projection's epilogue, the layout the attention kernel's PV product wants;
  * cross-attention K / V^T depend only on the text embeddings and are computed once per prompt set, not per step;
  * per-step scalars (timestep, context_guidance) live in device memory, so a whole forward can be captured in a hipGraph
    and replayed (capture=True) -- ~700 launches become one graph launch.
"""
import ctypes as CT
import weakref

import torch

from . import _lib as L
from . import ops
from .config import UNetConfig


class _Res:
    pass


class HipUNet:
    def __init__(self, cfg: UNetConfig, state, dtype=torch.bfloat16, device="cuda:0", x3=False, fp8_conv=False):
        """dtype float32 = exact-fp32 parity mode, bfloat16 = fast mode.  x3 (with dtype float32): the split-bf16 mode -- activations,
        norms, softmax and the residual stream stay fp32 exactly as in parity mode, every Linear / conv runs as an FFN_BF16X3 GEMM
        (hi/lo bf16 operands, three bf16 MFMAs per product term, fp32 accumulation; include/freefine_hip.h)."""
        assert not x3 or dtype == torch.float32, "split-bf16 mode keeps fp32 activations"
        assert not fp8_conv or dtype == torch.bfloat16, "fp8 convolutions are an option of the bf16 fast mode"
        self.x3 = bool(x3)
        # fp8_conv: the two 3x3 convolutions of every ResBlock take e4m3 operands (FFN_FP8): their inputs are SiLU(GroupNorm(.)) -- bounded,
        # written as fp8 by the norm's apply pass -- and their weights are quantised once with a per-tensor power-of-two scale.  Everything
        # else (attention, Linear layers, the residual stream) is the bf16 mode.  Reported beside the bf16 number, never as parity.
        self.fp8_conv = bool(fp8_conv)
        self.cfg, self.dtype, self.device = cfg, dtype, torch.device(device)
        self.in_channels = cfg.in_channels
        self.hook, self.controller = "edit", None
        self._graphs = {}
        self._capture_stream = None
        self._text_bufs = {}
        self.use_graph = False
        self._row_map = None
        self._plan_cache = {}
        self._row_idx = {}
        self._reuse, self._reuse_idx, self._enc_a, self.last_boundary = None, {}, {}, None
        self._in_phase_a = False
        self._kv_ext = False
        self.last_kv = None
        self._enc_rows = 0
        self.reuse_replays = 0             # forwards whose reference rows re-entered from a recorded state (tests / bench report it)
        self._pack(state)

    # ------------------------------------------------------------------------------------------------------------
    # weights
    # ------------------------------------------------------------------------------------------------------------
    def _f32(self, t):
        return t.detach().float().contiguous().to(self.device)

    def _lin(self, st, name, bias=True):
        w = st[name + ".weight"].to(self.device)
        if w.ndim == 4:
            w = w.reshape(w.shape[0], w.shape[1])
        return ops.pack_linear(w.float(), self.dtype, self.x3), (self._f32(st[name + ".bias"]) if bias else None), w.shape[1]

    def _conv(self, st, name, cin_pad=None):
        w = st[name + ".weight"].to(self.device)
        return ops.pack_conv3x3(w.float(), self.dtype, cin_pad, self.x3), self._f32(st[name + ".bias"]), (cin_pad or w.shape[1])

    def _resnet(self, st, p, temb_list):
        r = _Res()
        r.n1 = (self._f32(st[p + ".norm1.weight"]), self._f32(st[p + ".norm1.bias"]))
        r.n2 = (self._f32(st[p + ".norm2.weight"]), self._f32(st[p + ".norm2.bias"]))
        if self.fp8_conv:
            r.c1 = (ops.pack_conv3x3_f8(st[p + ".conv1.weight"].to(self.device).float()), self._f32(st[p + ".conv1.bias"]), st[p + ".conv1.weight"].shape[1])
            r.c2 = (ops.pack_conv3x3_f8(st[p + ".conv2.weight"].to(self.device).float()), self._f32(st[p + ".conv2.bias"]), st[p + ".conv2.weight"].shape[1])
        else:
            r.c1 = self._conv(st, p + ".conv1")
            r.c2 = self._conv(st, p + ".conv2")
        r.cout = st[p + ".conv1.weight"].shape[0]
        r.sc = self._lin(st, p + ".conv_shortcut") if (p + ".conv_shortcut.weight") in st else None
        r.temb_off = sum(w.shape[0] for w, _ in temb_list)
        temb_list.append((st[p + ".time_emb_proj.weight"].float(), st[p + ".time_emb_proj.bias"].float()))
        return r

    def _transformer(self, st, p, heads):
        t = _Res()
        t.heads = heads
        t.norm = (self._f32(st[p + ".norm.weight"]), self._f32(st[p + ".norm.bias"]))
        t.proj_in = self._lin(st, p + ".proj_in")
        t.proj_out = self._lin(st, p + ".proj_out")
        b = p + ".transformer_blocks.0"
        t.ln = [(self._f32(st[f"{b}.norm{i}.weight"]), self._f32(st[f"{b}.norm{i}.bias"])) for i in (1, 2, 3)]
        wq, wk = st[f"{b}.attn1.to_q.weight"].float(), st[f"{b}.attn1.to_k.weight"].float()
        t.C = wq.shape[0]
        t.w_qk1 = ops.pack_linear(torch.cat([wq, wk], 0).to(self.device), self.dtype, self.x3)          # self-attn Q|K in one GEMM
        t.w_v1 = ops.pack_linear(st[f"{b}.attn1.to_v.weight"].float().to(self.device), self.dtype, self.x3)
        t.o1 = self._lin(st, f"{b}.attn1.to_out.0")
        t.w_q2 = ops.pack_linear(st[f"{b}.attn2.to_q.weight"].float().to(self.device), self.dtype, self.x3)
        t.w_k2 = ops.pack_linear(st[f"{b}.attn2.to_k.weight"].float().to(self.device), self.dtype, self.x3)
        t.w_v2 = ops.pack_linear(st[f"{b}.attn2.to_v.weight"].float().to(self.device), self.dtype, self.x3)
        t.o2 = self._lin(st, f"{b}.attn2.to_out.0")
        t.ff1 = ops.pack_geglu(st[f"{b}.ff.net.0.proj.weight"].float().to(self.device), st[f"{b}.ff.net.0.proj.bias"].float().to(self.device), self.dtype, self.x3)
        t.ff2 = self._lin(st, f"{b}.ff.net.2")
        return t

    def _pack(self, st):
        cfg = self.cfg
        ch = cfg.block_out_channels
        n = len(ch)
        e = 8 if self.x3 else ops.epc(self.dtype)          # split-bf16: planes of whole 16-byte bf16 chunks
        self.cin_pad = (cfg.in_channels + e - 1) // e * e
        self.conv_in = self._conv(st, "conv_in", self.cin_pad)
        self.te1 = self._lin(st, "time_embedding.linear_1")
        self.te2 = self._lin(st, "time_embedding.linear_2")
        self.freq = ops.timestep_freqs(ch[0], self.device, shift=cfg.freq_shift)
        temb_list = []
        self.down, self.up = [], []
        self.attn_calls = 0
        for i in range(n):
            blk = _Res()
            blk.res = [self._resnet(st, f"down_blocks.{i}.resnets.{j}", temb_list) for j in range(cfg.layers_per_block)]
            blk.attn = [self._transformer(st, f"down_blocks.{i}.attentions.{j}", cfg.heads[i]) for j in range(cfg.layers_per_block)] \
                if cfg.down_has_attn[i] else None
            blk.down = self._conv(st, f"down_blocks.{i}.downsamplers.0.conv") if i < n - 1 else None
            self.down.append(blk)
        self.mid = _Res()
        self.mid.res = [self._resnet(st, "mid_block.resnets.0", temb_list)]
        self.mid.attn = [self._transformer(st, "mid_block.attentions.0", cfg.heads[n - 1])]
        self.mid.res.append(self._resnet(st, "mid_block.resnets.1", temb_list))
        rev_attn = list(reversed(cfg.down_has_attn))
        for i in range(n):
            blk = _Res()
            blk.res = [self._resnet(st, f"up_blocks.{i}.resnets.{j}", temb_list) for j in range(cfg.layers_per_block + 1)]
            blk.attn = [self._transformer(st, f"up_blocks.{i}.attentions.{j}", cfg.heads[n - 1 - i]) for j in range(cfg.layers_per_block + 1)] \
                if rev_attn[i] else None
            blk.up = self._conv(st, f"up_blocks.{i}.upsamplers.0.conv") if i < n - 1 else None
            blk.up2 = None                                  # the same convolution in its sub-pixel form (4/9 of the FLOPs): bf16 and split-bf16 modes
            if blk.up is not None and (self.dtype == torch.bfloat16 or self.x3):
                wu = st[f"up_blocks.{i}.upsamplers.0.conv.weight"].to(self.device)
                if ops.up2x_eligible(wu.shape[1], wu.shape[0], 192):
                    blk.up2 = ops.pack_conv3x3_up2x(wu, self.dtype, x3=self.x3)
            self.up.append(blk)
        self.norm_out = (self._f32(st["conv_norm_out.weight"]), self._f32(st["conv_norm_out.bias"]))
        self.conv_out = self._conv(st, "conv_out")
        # four output channels: a direct fp32 convolution on the vector ALU instead of 1/32 of an MFMA tile (ops.conv3x3_n4, round 5)
        wco = st["conv_out.weight"]
        self.conv_out_n4 = ops.pack_conv3x3_n4(wco.to(self.device)) if ops.conv3x3_n4_eligible(wco.shape[0], wco.shape[1]) else None
        # conv_out has out_channels (4) outputs: fine for the kernel (N % 4 == 0)
        wcat = torch.cat([w for w, _ in temb_list], 0).to(self.device)
        self.temb_w = ops.pack_linear(wcat, self.dtype, self.x3)
        self.temb_b = torch.cat([b for _, b in temb_list], 0).float().to(self.device).contiguous()
        self.transformers = [t for blk in self.down if blk.attn for t in blk.attn] + self.mid.attn + \
                            [t for blk in self.up if blk.attn for t in blk.attn]
        self.num_attention_calls = 2 * len(self.transformers)
        self.t_dev = torch.zeros(1, dtype=torch.float32, device=self.device)
        self.cg_dev = torch.zeros(1, dtype=torch.float32, device=self.device)

    _INSTANCE_STATE = ("hook", "controller", "_graphs", "_capture_stream", "_text_bufs", "use_graph", "_row_map", "_plan_cache", "_row_idx", "t_dev", "cg_dev",
                       "_reuse", "_reuse_idx", "_enc_a", "last_boundary", "last_kv")

    def share(self):
        """a second executor over the SAME packed weights with its own controller hook, device scalars, static buffers and
        graphs -- lets two edits run concurrently on two HIP streams (independent GeoBench cases) without doubling HBM use."""
        other = object.__new__(HipUNet)
        other.__dict__.update({k: v for k, v in self.__dict__.items() if k not in self._INSTANCE_STATE})
        other.hook, other.controller = "edit", None
        other._graphs, other._text_bufs, other._plan_cache, other._row_idx = {}, {}, {}, {}
        other._capture_stream = None
        other._reuse, other._reuse_idx, other._enc_a, other.last_boundary, other.last_kv = None, {}, {}, None, None
        other.use_graph, other._row_map = self.use_graph, None
        other.t_dev, other.cg_dev = torch.zeros_like(self.t_dev), torch.zeros_like(self.cg_dev)
        return other

    # ------------------------------------------------------------------------------------------------------------
    # reference-API surface
    # ------------------------------------------------------------------------------------------------------------
    def set_attention_control(self, hook, controller):
        """controller: one Attention_Modulator, or a list of them = an IMAGE-BATCHED forward: the batch holds len(list)
        independent edits, image-major (image i owns physical rows [i*Bp, (i+1)*Bp)); each controller plans its own rows."""
        self.hook, self.controller = hook, controller
        self._graphs.clear()
        self._plan_cache.clear()

    def _ctrls(self):
        c = self.controller
        return [] if c is None else (list(c) if isinstance(c, (list, tuple)) else [c])

    def to(self, *a, **k):
        return self

    def __call__(self, sample, timestep, encoder_hidden_states=None, row_map=None, reuse=None, **kw):
        return self.forward(sample, timestep, encoder_hidden_states, row_map, reuse)

    # ------------------------------------------------------------------------------------------------------------
    # text-side precompute: cross-attention K and V^T for all 16 blocks (constant across the sampling loop)
    # ------------------------------------------------------------------------------------------------------------
    def prepare_text(self, enc):
        """K and V^T of every cross-attention block for these text embeddings.  Buffers are static per embedding SHAPE
        (a captured graph keeps pointing at them); they are recomputed in place when a different tensor arrives."""
        key = tuple(enc.shape)
        ent = self._text_bufs.get(key)
        if ent is not None and ent["ref"]() is enc and ent["version"] == enc._version:
            return ent["kv"]
        Bt, Sk, Dm = enc.shape
        x = enc.to(self.device)
        x = ops.cast(x.float().contiguous(), self.dtype) if x.dtype != self.dtype else x.contiguous()
        ld = (Sk + 7) // 8 * 8
        old = ent["kv"] if ent is not None else [(None, None)] * len(self.transformers)
        kv = []
        for t, (ko, vo) in zip(self.transformers, old):
            k = ops.linear(x, t.w_k2, None, K=Dm, out=ko)
            vt = ops.linear(x, t.w_v2, None, K=Dm, rows_per_batch=Sk, transposed_ld=ld, out=vo)
            kv.append((k, vt))
        self._text_bufs[key] = dict(ref=weakref.ref(enc), version=enc._version, kv=kv)
        return kv

    # ------------------------------------------------------------------------------------------------------------
    # forward
    # ------------------------------------------------------------------------------------------------------------
    # ------------------------------------------------------------------------------------------------------------
    # reference-stream reuse ("stored reference K/V"): the guided loop's reference row UNet(x_ref, t_i, "") is the very
    # (latent, timestep, prompt) the inversion pass evaluated as its original-image row (model.py:582-586 vs :883), and nothing
    # modulates that row before the first TCA block (layer_idx starts at transformer block 10 = the first of up_blocks[2]; its cross
    # attention is plain, attention.py:1381-1383).  So the inversion forward RECORDS that row's state at the join point -- the hidden
    # state entering the up block that holds the first TCA layer and the skip tensors still to be consumed -- and the guided forward
    # REPLAYS it: conv_in ... up_blocks[join-1] run on the edit rows only, the reference row joins from the recorded state for
    # the remaining up blocks (where its K / V feed the edit rows).  Exact in exact arithmetic, like the CFG row de-duplication.
    # ------------------------------------------------------------------------------------------------------------
    def join_block(self, min_tca_block=None):
        """the up block at whose entrance the reference row may join: the last one whose first transformer block is <= the first
        modulated self-attention block (None = no modulated block: the last up block)"""
        n = len(self.up)
        tb = len([t for blk in self.down if blk.attn for t in blk.attn]) + 1
        first = []
        for blk in self.up:
            first.append(tb)
            tb += len(blk.attn) if blk.attn else 0
        if min_tca_block is None:
            return n - 1, first[n - 1]
        j = max([i for i in range(n) if first[i] <= min_tca_block], default=0)
        return j, first[j]

    def forward(self, sample, timestep, enc, row_map=None, reuse=None):
        """sample [B,Cin,h,w] fp32 (cuda), timestep int/0-d tensor, enc [Bt,77,D] -> eps [B,Cout,h,w] fp32.
        row_map (optional): the caller's LOGICAL batch has len(row_map) rows of which only the distinct ones were passed in
        (`sample`/`enc` hold the physical rows, row_map[logical] = physical): the attention controller still plans for the
        logical batch, its pass tables are translated, and the result is expanded back to the logical batch.
        reuse (optional, see above): dict(mode="record", join=j) -> after the call `self.last_boundary` holds the tensors at the
        entrance of up block j ([x, skip, skip, ...], all physical rows); dict(mode="replay", join=j, ref=[bool per physical row
        of ONE image], state=[tensors [n_ref_rows, HW, C] ...], drop_tail=bool) -> rows flagged `ref` skip everything before up block j
        and continue from `state`; the remaining blocks run on all rows.  drop_tail: the caller does not read the reference rows' eps
        (every guided step but the last overwrites their latent, model.py:582-586) -> those rows stop after the K / V projection of the
        last transformer block, the last thing any other row reads of them, and their eps rows come back as zeros.
        Stored reference K / V (hooks whose reference rows are NOT modulated -- composition: attention.py:1284-1324 leaves them plain):
        dict(mode="record", kv_from=t0) -> `self.last_kv` = [(K [B,S,C] view, V^T [B,C,S']) of transformer blocks t0, t0+1, ...];
        dict(mode="replay_kv", kv_from=t0, ref=[...], kv=[(K, V^T) of the reference rows, image-major, per recorded block],
        text_sel=[text rows of ONE image the surviving rows read, or None = their own]) -> rows flagged `ref` are not evaluated at all:
        the self attention of blocks >= t0 reads their K / V from `kv` (appended behind the computed rows), their eps rows are zeros."""
        sample = sample.to(self.device, torch.float32).contiguous()
        B = sample.shape[0]
        self._row_map = tuple(row_map) if row_map is not None else None
        self._enc_rows = enc.shape[0]
        self._reuse = self._prepare_reuse(reuse, B, enc)
        self.t_dev.fill_(float(timestep))
        ctrls = self._ctrls()
        assert not ctrls or B % len(ctrls) == 0, f"batch {B} is not a multiple of the {len(ctrls)} batched images"
        if ctrls and ctrls[0].context_guidance is not None:
            assert all(c.context_guidance == ctrls[0].context_guidance for c in ctrls), "batched images share one schedule"
            self.cg_dev.fill_(float(ctrls[0].context_guidance))
        text_kv = self.prepare_text(enc)
        ru = self._reuse
        if ru is not None and ru["mode"] in ("replay", "replay_kv"):
            ru["text_kv_a"] = self.prepare_text(ru["enc_a"])
            self.reuse_replays += 1
        if not self.use_graph:
            return self._expand(self._run(sample, text_kv))
        # graph mode: plan every attention call first (this also refreshes the controller's static mask vectors and
        # advances its counters exactly as an eager forward would); the plans' fingerprint is part of the graph key
        state = [(c.cur_att_layer, c.cur_step) for c in ctrls]
        fp = self._plan_all(B, sample.shape[2], sample.shape[3])
        rsig = None if ru is None else (ru["mode"], ru.get("join"), ru.get("kv_from"), ru.get("ref"), ru.get("text_sel"), bool(ru.get("drop_tail")),
                                        tuple(tuple(t.shape) for t in ru.get("state", ())))
        sig = (B, tuple(sample.shape), tuple(enc.shape), fp, self._row_map, len(ctrls), rsig)
        g = self._graphs.get(sig)
        if g is None:
            for c, st in zip(ctrls, state):
                c.cur_att_layer, c.cur_step = st
            g = self._capture(sample, text_kv, sig)
        g["x"].copy_(sample)
        if ru is not None and ru["mode"] in ("replay", "replay_kv"):      # the recorded reference state of THIS step into the graph's static inputs
            assert len(g["ref_in"]) == len(ru["state"])
            for dst, src in zip(g["ref_in"], ru["state"]):
                dst.copy_(src)
        self._launch(g)
        if ru is not None and ru["mode"] == "record":
            self.last_boundary, self.last_kv = g["boundary"], g["kv"]
        return self._expand(g["out"].clone())

    def features(self, sample, timestep, enc, up_ft_index):
        """The activations at the end of up block `up_ft_index` -- diffusers' block boundary, the block's upsampler included, which is what DIFT records
        (the reference's evaluation/metrics/MD/dift_sd.py:124-155); nothing after that block is executed.  sample [B,Cin,h,w] fp32, enc [B,77,D] ->
        (rows [B, H*W, C] in the activation dtype, (H, W)).  The rows are returned where the executor left them: an up block that is not the last writes
        its output into the left columns of the next concatenation buffer, so rows.stride(1) may exceed C (no copy is made).  Plain attention whatever
        controller is registered (it is set aside for the call and put back), none of the reuse modes, always eager: no graph is captured or replayed.
        State shared with forward(): the per-call fields `_row_map`, `_reuse`, `_enc_rows` and the device timestep `t_dev` are overwritten, and the static
        per-shape text K / V buffers (which captured graphs point at) are recomputed in place for `enc`; forward() sets the former on every call and
        prepare_text re-projects the latter as soon as another tensor arrives, so a forward() after features() computes what it did before.
        Batch invariance: the launch choices taken from the number of rows are pinned (ops.batch_invariant: no K split, GroupNorm in the form of one row) and
        the upsamplers run as plain convolutions (the sub-pixel form is chosen by the row count).  The tile of an unsplit GEMM still follows M; a tile
        changes which workgroup computes an element, not the K order of its accumulation.  Tested: a row's features are bit-identical at 6, 24 and 48 rows
        on the tiny topology in all three modes, across the GroupNorm threshold (tests/test_dift_gpu.py).  Beyond what is tested -- the SD-2.1 size has
        not been measured -- this is a property the pinned choices are meant to give, not a guarantee of the library."""
        n = len(self.up)
        assert isinstance(up_ft_index, int) and 0 <= up_ft_index < n, f"up_ft_index {up_ft_index} outside [0, {n})"
        sample = sample.to(self.device, torch.float32).contiguous()
        ctrl, self.controller = self.controller, None
        try:
            self._row_map, self._reuse, self._enc_rows = None, None, enc.shape[0]
            self.t_dev.fill_(float(timestep))
            with ops.batch_invariant():
                x, H, W = self._run(sample, self.prepare_text(enc), stop_up=up_ft_index)
        finally:
            self.controller = ctrl
        return x, (H, W)

    @staticmethod
    def _launch(g):
        """replay a captured forward.  Through the C ABI (ffn_graph_launch = hipGraphLaunch on the current stream): a ctypes call releases the GIL,
        torch's CUDAGraph.replay() holds it -- and a launch of the ~380-node graph keeps the host thread for milliseconds on ROCm 7.2 (measured:
        5.2 ms per replay, profiles/r5_host_profile_batch1.txt), which serialised the host threads of the one-image-per-call layout.  The graphs
        hold no torch RNG state, so the raw launch is the whole of replay()."""
        if hasattr(g["graph"], "raw_cuda_graph_exec"):          # (older torch: no raw handle -> torch's replay())
            ex = g.get("exec")
            if ex is None:
                ex = g["exec"] = int(g["graph"].raw_cuda_graph_exec())
            # replay()'s device guard, kept: the graph runs on the device it was captured on, on THAT device's current stream
            with torch.cuda.device(g.get("device", torch.cuda.current_device())):
                L.check(L.load().ffn_graph_launch(CT.c_void_p(torch.cuda.current_stream().cuda_stream), CT.c_void_p(ex)), "ffn_graph_launch")
        else:
            g["graph"].replay()

    def _prepare_reuse(self, reuse, B, enc):
        if reuse is None:
            return None
        ru = dict(reuse)
        K = max(1, len(self._ctrls()))
        Bp = B // K
        if ru["mode"] == "replay_kv":                          # flat list of the recorded tensors in the order _run consumes them
            ru["kv_from"] = int(ru["kv_from"])
            assert len(ru["kv"]) == len(self.transformers) - ru["kv_from"], (len(ru["kv"]), ru["kv_from"])
            ru["state"] = [t for kv in ru["kv"] for t in kv]
            ru["text_sel"] = None if ru.get("text_sel") is None else tuple(int(r) for r in ru["text_sel"])
        if ru["mode"] in ("replay", "replay_kv"):
            ref = tuple(bool(r) for r in ru["ref"])
            assert len(ref) == Bp and any(ref) and not all(ref), (ref, Bp)
            ru["ref"] = ref
            ru["sel"] = [p for p in range(Bp) if not ref[p]]                 # physical rows (of one image) that run the whole net
            ru["refs"] = [p for p in range(Bp) if ref[p]]                    # ... whose state / K / V comes from the record
            key = (B, ref)
            ent = self._reuse_idx.get(key)
            if ent is None:
                sel, nr = ru["sel"], sum(ref)
                idx_a = [i * Bp + p for i in range(K) for p in sel]
                # rows of cat([phase-A rows (image-major), recorded reference rows (image-major)]) in physical order
                perm, ra, rr = [], 0, 0
                for i in range(K):
                    a0, r0, ia, ir = i * len(sel), K * len(sel) + i * nr, 0, 0
                    for p in range(Bp):
                        if ref[p]:
                            perm.append(r0 + ir); ir += 1
                        else:
                            perm.append(a0 + ia); ia += 1
                ent = self._reuse_idx[key] = (torch.tensor(idx_a, device=self.device), torch.tensor(perm, device=self.device))
            ru["idx_a"], ru["perm"] = ent
            ru["idx_a_list"] = [i * Bp + p for i in range(K) for p in ru["sel"]]
            tsel = ru.get("text_sel")
            ck = (id(enc), enc._version, key, tsel)
            ea = self._enc_a.get(ck)
            if ea is None or ea[0]() is not enc:
                if len(self._enc_a) > 8:
                    self._enc_a.clear()
                if tsel is None:                              # text rows aligned with the latent rows: the surviving rows' own
                    tidx = ru["idx_a"]
                else:                                         # composition hook: R + 1 + P text rows per image, `text_sel` of them survive
                    assert enc.shape[0] % K == 0
                    bt = enc.shape[0] // K
                    tidx = torch.tensor([i * bt + r for i in range(K) for r in tsel], device=self.device)
                ea = self._enc_a[ck] = (weakref.ref(enc), enc.to(self.device).index_select(0, tidx).contiguous())
            ru["enc_a"] = ea[1]
        return ru

    def _expand(self, eps):
        if self._row_map is None:
            return eps
        rm, K = self._row_map, max(1, len(self._ctrls()))
        idx = self._row_idx.get((rm, K))
        if idx is None:                                   # device-side index: no per-step host->device copy / sync
            Bp = eps.shape[0] // K
            idx = self._row_idx[(rm, K)] = torch.tensor([i * Bp + r for i in range(K) for r in rm], device=self.device)
        return eps.index_select(0, idx)

    REF_KV = 1 << 20                                           # kv_row of a RECORDED reference row inside a per-image plan: REF_KV + its index among the image's reference rows

    def _plan_one(self, c, is_cross, place, B, S, heads, sel=None, refs=None, tsel=None):
        """one controller's plan for its logical batch, translated to its physical (deduplicated) rows.  B = physical rows of
        the image; sel (reference-stream reuse) = the subset of them present in this launch, in launch order; refs (stored reference
        K / V, self attention of a recorded block) = the image's recorded rows, which a term may name as its K / V row but not as its
        Q row; tsel (cross attention whose text batch is not row-aligned with the latent batch) = the text rows of the image present
        in this launch."""
        rm = self._row_map
        plan = c.plan(self.hook, is_cross, place, len(rm) if rm is not None else B, S, heads, self.device)
        if plan["passes"] is None or (rm is None and sel is None):
            return plan
        plan = dict(plan)
        if rm is not None:
            rep = [rm.index(pr) for pr in range(B)]        # representative logical row of every physical row
            plan["passes"] = [[None if rows[l] is None else rows[l].remap(rm, l) for l in rep] for rows in plan["passes"]]
            if "ref_rows" in plan:
                plan["ref_rows"] = [rm[plan["ref_rows"][l]] for l in rep]
        else:                                              # physical = logical rows (the K / V rows may index a text batch of another size):
            plan["passes"] = [[None if e is None else e.pinned(l) for l, e in enumerate(rows)] for rows in plan["passes"]]      # only pin the head rule
        assert sel is None or "ref_rows" not in plan, "shared-K/V (style-align) attention cannot run on a row subset"
        if sel is not None:
            ren = {p: a for a, p in enumerate(sel)}
            kv_ren = ren
            if is_cross and tsel is not None:
                kv_ren = {r: a for a, r in enumerate(tsel)}
            elif refs is not None:
                kv_ren = dict(ren)
                kv_ren.update({p: self.REF_KV + j for j, p in enumerate(refs)})
            plan["passes"] = [[None if rows[p] is None else rows[p].renumber(ren, kv_ren) for p in sel] for rows in plan["passes"]]
        return plan

    def _phase(self, B):
        """(physical rows per image the controllers plan for, subset of them present in the CURRENT launch or None, the image's recorded
        rows this attention call may read K / V of or None, the image's text rows present or None = aligned with the latent rows) --
        phase A of a replayed forward, and the whole of a stored-K/V forward, hold only the non-reference rows"""
        K = max(1, len(self._ctrls()))
        ru = self._reuse
        if ru is not None and ru["mode"] == "replay" and self._in_phase_a:
            return len(ru["ref"]), ru["sel"], None, None
        if ru is not None and ru["mode"] == "replay_kv":
            return len(ru["ref"]), ru["sel"], (ru["refs"] if self._kv_ext else None), ru["text_sel"]
        return B // K, None, None, None

    def _plan(self, is_cross, place, B, S, heads):
        """plan of this attention call for the whole physical batch.  Image-batched forwards: every image's controller plans
        its own Bp rows; the tables are concatenated with the image's row offset, the tiled-head rule pinned to the row index
        the image would have had alone (attention.py:859 vs 761 depend on b*heads+head).  Stored-K/V forwards: the K / V rows of a
        recorded block's self attention are [computed rows, image-major | recorded reference rows, image-major]."""
        ctrls = self._ctrls()
        Bp, sel, refs, tsel = self._phase(B)
        K = len(ctrls)
        plans = [self._plan_one(c, is_cross, place, Bp, S, heads, sel, refs, tsel) for c in ctrls]
        if K == 1 and sel is None:
            return plans[0]
        if all(p["passes"] is None for p in plans):
            return plans[0]
        assert len({p["kind"] for p in plans}) == 1, "batched images must take the same attention branch kind"
        rm = self._row_map
        rep = [rm.index(pr) for pr in range(Bp)] if rm is not None else list(range(Bp))
        if sel is not None:
            rep = [rep[p] for p in sel]
        Bp = len(rep)                                          # rows per image in this launch
        nr = len(refs) if refs is not None else 0
        npass = max(len(p["passes"]) for p in plans if p["passes"] is not None)
        merged = [[] for _ in range(npass)]
        # cross attention reads K / V rows of the TEXT batch: image i's block starts at i * (text rows per image), which differs from
        # its latent rows only under the composition hook (R + 1 + P text rows for R + 2 latent rows)
        if is_cross and sel is not None and tsel is not None:
            Bt = len(tsel)
        else:
            Bt = (self._enc_rows // K) if (is_cross and sel is None and self._enc_rows % K == 0) else Bp
        for i, plan in enumerate(plans):
            ps = plan["passes"] if plan["passes"] is not None else [[ops.AttnEntrySpec(b, b) for b in range(Bp)]]
            for p in range(npass):
                rows = ps[p] if p < len(ps) else [None] * Bp
                for pr, e in enumerate(rows):
                    if e is not None:
                        ref_j = e.kv_row - self.REF_KV
                        e = e.shifted(i * Bp, rep[pr], i * Bt)
                        if ref_j >= 0:                          # a recorded row: behind all K * Bp computed ones
                            e.kv_row = K * Bp + i * nr + ref_j
                    merged[p].append(e)
        out = dict(kind=plans[0]["kind"], passes=merged, needs_cg=any(p["needs_cg"] for p in plans),
                   branch="+".join(sorted({p.get("branch", "") for p in plans})))
        if any("ref_rows" in p for p in plans):
            out["ref_rows"] = [i * Bp + r for i, p in enumerate(plans) for r in p.get("ref_rows", list(range(Bp)))]
        return out

    def _call_list(self, H, W):
        """(is_cross, place, S, heads) of every attention call in execution order."""
        cfg = self.cfg
        n = len(cfg.block_out_channels)
        out = []
        h, w = H, W
        for i in range(n):
            if cfg.down_has_attn[i]:
                out += [(x, "down", h * w, cfg.heads[i]) for _ in range(cfg.layers_per_block) for x in (False, True)]
            if i < n - 1:
                h, w = (h + 1) // 2, (w + 1) // 2
        out += [(False, "mid", h * w, cfg.heads[n - 1]), (True, "mid", h * w, cfg.heads[n - 1])]
        rev_attn = list(reversed(cfg.down_has_attn))
        for i in range(n):
            if rev_attn[i]:
                out += [(x, "up", h * w, cfg.heads[n - 1 - i]) for _ in range(cfg.layers_per_block + 1) for x in (False, True)]
            if i < n - 1:
                h, w = 2 * h, 2 * w
        return out

    def _ctrl_key(self, B, H, W):
        """everything a forward's attention plans depend on (masks by identity + in-place version)"""
        ru = self._reuse
        key = [self.hook, B, H, W, self._row_map,
               None if ru is None or ru["mode"] == "record" else (ru["mode"], ru.get("join"), ru.get("kv_from"), ru["ref"], ru.get("text_sel"), bool(ru.get("drop_tail")))]
        for c in self._ctrls():
            mv = tuple((m.data_ptr(), m._version) if torch.is_tensor(m) else None
                       for m in (c.fg_retain_mask, c.fg_ref_mask, c.local_edit_region, c.src_masks, c.tgt_masks))
            key.append((id(c), c.use_tca, c.use_style_align, c.local_edit, c.method, tuple(c.layer_idx), tuple(c.tca_scope),
                        tuple(c.style_align_scope), c.cur_att_layer, c.prompt_length, c._mask_epoch, mv))
        return tuple(key)

    def _plan_all(self, B, H, W):
        ctrls = self._ctrls()
        if not ctrls:
            return None
        key = self._ctrl_key(B, H, W)
        hit = self._plan_cache.get(key)
        if hit is not None:                      # nothing the plans depend on changed: only advance the counters
            for c in ctrls:
                c.cur_step += 1 if c.cur_att_layer == 0 else 0
                if c.cur_att_layer != 0:
                    for _ in range(self.num_attention_calls):
                        c._tick()
            return hit
        fp = self._plan_all_slow(B, H, W)
        if len(self._plan_cache) > 64:
            self._plan_cache.clear()
        self._plan_cache[key] = fp
        return fp

    def _plan_all_slow(self, B, H, W):
        fps = []
        ru = self._reuse
        join_tb = self.join_block_tb(ru["join"]) if (ru is not None and ru["mode"] == "replay") else -1
        kv_from = ru["kv_from"] if (ru is not None and ru["mode"] == "replay_kv") else None
        calls = self._call_list(H, W)
        drop = ru is not None and ru["mode"] == "replay" and bool(ru.get("drop_tail"))
        for ci, (is_cross, place, S, heads) in enumerate(calls):
            self._in_phase_a = ci // 2 < join_tb             # phase A of a replayed forward: the non-reference rows only
            self._kv_ext = kv_from is not None and not is_cross and ci // 2 >= kv_from      # stored K / V: self attention of a recorded block
            if drop and ci == len(calls) - 1:                 # dropped tail: the last block's cross attention runs on the non-reference rows
                self._in_phase_a = True
            plan = self._plan(is_cross, place, B, S, heads)
            if drop and ci == len(calls) - 2:                 # ... and its self attention has no reference QUERY rows
                plan = self._without_ref_queries(plan, B)
            if plan["passes"] is None:
                fps.append(0)
                continue
            rows = tuple(tuple(None if e is None else (e.q_row, e.kv_row, e.w_const, e.w_slope, e.flags, e.hr_row,
                                                       0 if e.wq is None else e.wq.data_ptr(),
                                                       0 if e.kmask is None else e.kmask.data_ptr(),
                                                       0 if e.qsel is None else e.qsel.data_ptr()) for e in r) for r in plan["passes"])
            fps.append((plan["kind"], plan["needs_cg"], rows))
        self._in_phase_a = self._kv_ext = False
        return (self.hook, tuple(fps))

    def join_block_tb(self, join):
        """index of the first transformer block of up block `join` (attention calls 2 * that and later belong to phase B)"""
        tb = len([t for blk in self.down if blk.attn for t in blk.attn]) + 1
        for blk in self.up[:join]:
            tb += len(blk.attn) if blk.attn else 0
        return tb

    def _capture(self, sample, text_kv, sig):
        ctrls = self._ctrls()
        state = [(c.cur_att_layer, c.cur_step) for c in ctrls]
        x_static = sample.clone()
        ru = self._reuse
        ref_in = None
        if ru is not None and ru["mode"] == "replay":          # static inputs for the recorded reference state (refilled before every replay)
            ref_in = [t.clone() for t in ru["state"]]
            ru["state_run"] = ref_in
        if ru is not None and ru["mode"] == "replay_kv":       # static K / V buffers whose reference rows are refilled before every replay:
            ref_in = ru["static"] = []                         # allocated (and filled) by the warm-up run below, found again by the captured one
            ru["static_bufs"] = []
        # warm-up outside capture (lazy module loading, LDS opt-ins, first upload of mask vectors), counters restored after
        self._run(x_static, text_kv)
        if ru is not None and ru["mode"] == "replay_kv":
            ru["static_ready"] = True
        for c, st in zip(ctrls, state):
            c.cur_att_layer, c.cur_step = st
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        # captured on this executor's own stream, not torch's one default capture stream: ops._workspace picks the split-K scratch by
        # stream, and executors whose graphs replay concurrently on different streams (share()) must not bake in the same buffer
        if self._capture_stream is None:
            self._capture_stream = torch.cuda.Stream(device=x_static.device)
        with torch.cuda.graph(graph, stream=self._capture_stream):
            out = self._run(x_static, text_kv)
        rec = ru is not None and ru["mode"] == "record"
        g = dict(graph=graph, x=x_static, out=out, ref_in=ref_in, ref_bufs=ru.get("static_bufs") if ru is not None else None,
                 boundary=self.last_boundary if rec else None, kv=self.last_kv if rec else None, device=x_static.device.index)
        if ru is not None:
            for k in ("state_run", "static", "static_bufs", "static_ready"):
                ru.pop(k, None)
        self._graphs[sig] = g
        return g

    def _gn(self, x, gb, eps, silu):
        B, HW, C = x.shape
        # split-bf16 mode: every GroupNorm / LayerNorm feeds a GEMM -> written directly in the [hi | lo] pair form that GEMM reads
        return ops.groupnorm(x, gb[0], gb[1], self.cfg.norm_num_groups, eps, silu=silu, pair=self.x3)

    def _gn_conv_in(self, x, gb, w):
        """SiLU(GroupNorm(x)) in the form the convolution `w` reads: e4m3 bytes (fp8 conv), pair rows (split-bf16) or the activation dtype"""
        if ops.is_f8(w):
            return ops.groupnorm_f8(x, gb[0], gb[1], self.cfg.norm_num_groups, self.cfg.norm_eps, w._ffn_f8[0], silu=True)
        return self._gn(x, gb, self.cfg.norm_eps, True)

    def _resblock(self, r, x, B, H, W, temb_all, out=None):
        cin = x.shape[-1]
        if r.sc is not None and self.x3 and not ops.is_f8(r.c1[0]) and ops.pair_width(x) is None and x.dtype == torch.float32:
            # split-bf16, ResBlock with a 1x1 shortcut: norm1's apply pass also writes the pair rows of x the shortcut GEMM reads (no ffn_split_pair pass)
            h, x = ops.groupnorm_pair_raw(x, r.n1[0], r.n1[1], self.cfg.norm_num_groups, self.cfg.norm_eps, silu=True)
        else:
            h = self._gn_conv_in(x, r.n1, r.c1[0])
        rb = temb_all[:, r.temb_off:r.temb_off + r.cout]
        h = ops.conv3x3(h, r.c1[0], r.c1[1], B, H, W, cin, rowbias=rb, rowbias_ld=temb_all.shape[1])
        h = self._gn_conv_in(h, r.n2, r.c2[0])
        if r.sc is not None:
            x = ops.linear(x, r.sc[0], r.sc[1], K=cin)
        return ops.conv3x3(h, r.c2[0], r.c2[1], B, H, W, r.cout, residual=x, out=out)

    def _without_ref_queries(self, plan, B):
        """the plan of a self-attention call over all B physical rows, restricted to the output rows that are not reference rows (dropped
        tail of a replayed forward): entries keep naming physical Q / K / V rows; the tiled-head rule stays pinned to the row it had"""
        keep = self._reuse["idx_a_list"]
        passes = plan["passes"] if plan["passes"] is not None else [[ops.AttnEntrySpec(b, b) for b in range(B)]]
        pin = lambda e, r: e if (e is None or e.hr_row is not None) else ops.AttnEntrySpec(e.q_row, e.kv_row, e.w_const, e.w_slope, e.wq, e.kmask, e.qsel, e.flags, r)
        out = dict(plan)
        out["passes"] = [[pin(rows[r], r) for r in keep] for rows in passes]
        return out

    def _self_plan(self, t, place, B, S, drop_ref_queries=False):
        """plan of a block's self attention, made BEFORE its K / V^T projections run (the controllers' layer counters advance once per attention
        call, in call order): None without a controller and without dropped rows"""
        if self.controller is None:
            return dict(kind="plain", needs_cg=False, passes=[[ops.AttnEntrySpec(r, r, hr_row=r) for r in self._reuse["idx_a_list"]]]) if drop_ref_queries else None
        plan = self._plan(False, place, B, S, t.heads)
        if drop_ref_queries:
            assert plan["kind"] != "shared_kv"
            plan = self._without_ref_queries(plan, B)
        return plan

    def _attention(self, t, is_cross, place, q, k, vt, ldq_view, B, S, Sk, plan=None, kv_images=False):
        """plan: a self-attention plan made by _self_plan (cross attention plans here)"""
        D = t.C // t.heads
        scale = D ** -0.5
        if is_cross and self.controller is not None:
            plan = self._plan(is_cross, place, B, S, t.heads)
        if plan is None:
            return ops.attention(q, k, vt, t.heads, scale, None, Sk=Sk, C=t.C, x3=self.x3, out_pair=self.x3, kv_images=kv_images)
        if plan["kind"] == "shared_kv":
            assert not kv_images
            rr = plan["ref_rows"]
            kc = k[..., :t.C] if k.shape[-1] != t.C else k
            k2 = torch.cat([kc, kc[rr]], dim=1).contiguous()                 # device-memory plumbing (non-default SSA/SDSA path)
            vt2 = torch.cat([vt[..., :Sk], vt[rr][..., :Sk]], dim=2).contiguous()
            return ops.attention(q, k2, vt2, t.heads, scale, plan["passes"], Sk=2 * Sk, C=t.C, x3=self.x3, out_pair=self.x3)
        return ops.attention(q, k, vt, t.heads, scale, plan["passes"], Sk=Sk, C=t.C, w_dev=self.cg_dev if plan["needs_cg"] else None, x3=self.x3,
                             out_pair=self.x3, kv_images=kv_images)

    def _kv_buffers(self, B, S, C, ldv):
        """stored-K/V forward, next recorded block: (q|k [B + n_ref, S, 2C], V^T [B + n_ref, C, ldv]) whose last n_ref rows hold the recorded
        K / V^T of the reference rows (the q half of those rows is never read).  Eager: allocated and filled here.  Graph: allocated and
        filled by the warm-up run -- the reference rows are static inputs which HipUNet.forward refills before every replay -- and
        found again by the captured run."""
        ru = self._reuse
        i = ru["cursor"]
        ru["cursor"] = i + 1
        if ru.get("static_ready"):
            return ru["static_bufs"][i]
        k_ref, vt_ref = ru["state"][2 * i], ru["state"][2 * i + 1]
        nr = k_ref.shape[0]
        assert tuple(k_ref.shape) == (nr, S, C) and tuple(vt_ref.shape) == (nr, C, ldv), (tuple(k_ref.shape), tuple(vt_ref.shape), (S, C, ldv))
        qk = torch.empty(B + nr, S, 2 * C, dtype=self.dtype, device=self.device)
        vt = torch.empty(B + nr, C, ldv, dtype=self.dtype, device=self.device)
        qk[B:, :, C:].copy_(k_ref)
        vt[B:].copy_(vt_ref)
        if ru.get("static") is not None:
            ru["static_bufs"].append((qk, vt))
            ru["static"] += [qk[B:, :, C:], vt[B:]]
        return qk, vt

    def _transformer_block(self, t, x, B, H, W, place, kv_text, out=None, drop=None, tb=0):
        """drop (dropped tail of a replayed forward, last block only) = (device index of the rows that go on, their cross-attention K / V):
        the reference rows stop once their K / V^T are projected.  tb = index of this transformer block (stored reference K / V)."""
        S, C = H * W, t.C
        res0 = x
        ru = self._reuse
        h = self._gn(x, t.norm, 1e-6, False)
        h = ops.linear(h, t.proj_in[0], t.proj_in[1], K=C)
        # --- self attention
        y = ops.layernorm(h, *t.ln[0], pair=self.x3)
        ldv = (S + 7) // 8 * 8
        if ru is not None and ru["mode"] == "replay_kv" and tb >= ru["kv_from"]:
            # recorded block of a stored-K/V forward: K / V^T hold the B computed rows followed by the recorded reference rows
            qk, vt = self._kv_buffers(B, S, C, ldv)
            ops.linear(y, t.w_qk1, None, K=C, out=qk[:B])
            ops.linear(y, t.w_v1, None, K=C, rows_per_batch=S, transposed_ld=ldv, out=vt[:B])
            self._kv_ext = True
            a = self._attention(t, False, place, qk[:B], qk[..., C:], vt, 2 * C, B, S, S, plan=self._self_plan(t, place, B, S))
            self._kv_ext = False
        else:
            plan = self._self_plan(t, place, B, S, drop_ref_queries=drop is not None)
            rec = ru is not None and ru["mode"] == "record" and ru.get("kv_from") is not None and tb >= ru["kv_from"]
            # split-bf16: the K and V^T projections write the attention kernel's pre-split [hi | lo] images in the bytes of the fp32 values they replace
            # (no ffn_attn_presplit pass).  Not for recorded K / V (a later stored-K/V forward reads them as fp32, under a plan unknown here) nor for
            # the shared-K/V plans (their K / V are gathered as fp32 tensors).
            img = self.x3 and not rec and (plan is None or plan["kind"] != "shared_kv") and \
                ops.kv_images_ok(C // t.heads, S, S, None if plan is None else plan["passes"], B * max(S * 2 * C, C * ldv) * 4)
            qk = ops.linear(y, t.w_qk1, None, K=C, kv64_from=C if img else None)        # [B,S,2C]: q | k
            vt = ops.linear(y, t.w_v1, None, K=C, rows_per_batch=S, transposed_ld=ldv, kv64_from=0 if img else None)           # V^T [B,C,S]
            if rec:
                self.last_kv.append((qk[..., C:], vt))
            a = self._attention(t, False, place, qk, qk[..., C:], vt, 2 * C, B, S, S, plan=plan, kv_images=img)
        if drop is not None:                                 # `a` already holds the surviving rows only; the residual streams follow
            idx, kv_text = drop
            h, res0, B = h.index_select(0, idx), res0.index_select(0, idx), idx.shape[0]
            self._in_phase_a = True
        h = ops.linear(a, t.o1[0], t.o1[1], K=C, residual=h)
        # --- cross attention
        y = ops.layernorm(h, *t.ln[1], pair=self.x3)
        q = ops.linear(y, t.w_q2, None, K=C)
        k2, vt2 = kv_text
        a = self._attention(t, True, place, q, k2, vt2, C, B, S, k2.shape[1])
        h = ops.linear(a, t.o2[0], t.o2[1], K=C, residual=h)
        # --- feed forward (GEGLU fused in the first GEMM's epilogue)
        y = ops.layernorm(h, *t.ln[2], pair=self.x3)
        y = ops.linear(y, t.ff1[0], t.ff1[1], K=C, geglu=True, out_pair=self.x3)
        # (the block's last residual sum feeds proj_out only: split-bf16 mode writes it as the pair rows that GEMM reads, no ffn_split_pair pass)
        h = ops.linear(y, t.ff2[0], t.ff2[1], K=4 * C, residual=h, out_pair=self.x3 and C % 32 == 0)
        return ops.linear(h, t.proj_out[0], t.proj_out[1], K=C, residual=res0, out=out)

    def _run(self, sample, text_kv, stop_up=None):
        """stop_up (HipUNet.features): return (activation rows, H, W) at the end of up block `stop_up`, its upsampler included, instead of eps; the
        upsamplers then take the plain convolution whatever the batch (the sub-pixel form is chosen by the row count and sums in another order)"""
        cfg = self.cfg
        B, _, H, W = sample.shape
        dt = self.dtype
        ru = self._reuse
        replay = ru is not None and ru["mode"] == "replay"
        record = ru is not None and ru["mode"] == "record"
        replay_kv = ru is not None and ru["mode"] == "replay_kv"
        BB = B                                                # rows of the whole launch (phase B)
        if replay:                                            # phase A: everything before up block `join` on the non-reference rows
            sample = sample.index_select(0, ru["idx_a"])
            B = sample.shape[0]
            text_kv = list(ru["text_kv_a"][:self.join_block_tb(ru["join"])]) + list(text_kv[self.join_block_tb(ru["join"]):])
        if replay_kv:                                         # stored reference K / V: the whole network on the non-reference rows
            sample = sample.index_select(0, ru["idx_a"])
            B = sample.shape[0]
            text_kv = ru["text_kv_a"]
            ru["cursor"] = 0
        if record and ru.get("kv_from") is not None:
            self.last_kv = []                                 # (K, V^T) of the recorded blocks, appended by _transformer_block
        self._in_phase_a = replay
        ti = iter(text_kv)
        tb = 0                                                # transformer block counter
        # time embedding -> silu(emb) -> all 22 resnet projections in one GEMM (fp32 row biases)
        te = ops.timestep_embed(self.t_dev, self.freq, BB, dt, flip=cfg.flip_sin_to_cos)      # (every row carries the same timestep)
        e1 = ops.linear(te, self.te1[0], self.te1[1], K=self.te1[2], silu=True)
        e2 = ops.linear(e1, self.te2[0], self.te2[1], K=self.te2[2], silu=True)     # = silu(time_embedding(t_emb))
        temb_all = ops.linear(e2, self.temb_w, self.temb_b, K=self.te2[0].shape[0], out_f32=True)
        temb_full = temb_all
        temb_all = temb_all[:B]
        x = ops.pack_nchw(sample, list(range(B)), self.cin_pad, dt)
        x = ops.conv3x3(x, self.conv_in[0], self.conv_in[1], B, H, W, self.cin_pad)
        skips = [(x, H, W)]
        n = len(self.down)
        for i, blk in enumerate(self.down):
            for j, r in enumerate(blk.res):
                x = self._resblock(r, x, B, H, W, temb_all)
                if blk.attn:
                    x = self._transformer_block(blk.attn[j], x, B, H, W, "down", next(ti), tb=tb)
                    tb += 1
                skips.append((x, H, W))
            if blk.down is not None:
                C = x.shape[-1]
                x = ops.conv3x3(x, blk.down[0], blk.down[1], B, H, W, C, stride=2)
                H, W = (H + 1) // 2, (W + 1) // 2
                skips.append((x, H, W))
        x = self._resblock(self.mid.res[0], x, B, H, W, temb_all)
        x = self._transformer_block(self.mid.attn[0], x, B, H, W, "mid", next(ti), tb=tb)
        tb += 1
        # Up path: whatever produces the input of a skip concatenation writes it straight into the left columns of the concatenated
        # buffer (ldo = C1 + C2), so the concat only copies the skip tensor
        def cat_dst(C1, HW):
            return ops.cat_dst((B, HW), C1, skips[-1][0].shape[-1], dt, x.device) if skips else None
        x = self._resblock(self.mid.res[1], x, B, H, W, temb_all, out=cat_dst(self.mid.res[1].cout, H * W))
        for i, blk in enumerate(self.up):
            if ru is not None and ru.get("join") is not None and i == ru["join"]:
                if record:                                    # the state every row enters up block `join` with: [x, skips still to be consumed (top of stack first)]
                    self.last_boundary = [x] + [s for s, _, _ in reversed(skips)]
                if replay:                                    # the reference rows join: recorded state + phase-A rows -> physical row order
                    state = ru.get("state_run") or ru["state"]
                    assert len(state) == 1 + len(skips), (len(state), len(skips))
                    merge = lambda a, r: torch.cat([a, r.to(a.dtype)], 0).index_select(0, ru["perm"])
                    x = merge(x, state[0])
                    skips = [(merge(s, st), sh, sw) for (s, sh, sw), st in zip(skips, reversed(state[1:]))]
                    B, temb_all = BB, temb_full
                    self._in_phase_a = False
            for j, r in enumerate(blk.res):
                s, sh, sw = skips.pop()
                assert (sh, sw) == (H, W)
                x = ops.concat(x, s)
                dst = cat_dst(r.cout, H * W) if j + 1 < len(blk.res) else None      # the next resblock of this block concatenates again
                x = self._resblock(r, x, B, H, W, temb_all, out=None if blk.attn else dst)
                if blk.attn:
                    last = replay and bool(ru.get("drop_tail")) and blk.attn[j] is self.transformers[-1]
                    drop = (ru["idx_a"], ru["text_kv_a"][-1]) if last else None
                    x = self._transformer_block(blk.attn[j], x, B, H, W, "up", next(ti), out=dst, drop=drop, tb=tb)
                    tb += 1
                    if last:                                  # from here on only the non-reference rows exist
                        assert dst is None and i == len(self.up) - 1 and j == len(blk.res) - 1, "the last transformer block closes the network"
                        B, temb_all = x.shape[0], temb_full[:x.shape[0]]
            if blk.up is not None:
                C = x.shape[-1]
                if blk.up2 is not None and stop_up is None and ops.up2x_eligible(C, C, B * H * W):
                    x = ops.conv3x3_up2x(x, blk.up2, blk.up[1], B, H, W, C, out=cat_dst(C, 4 * H * W))
                else:
                    x = ops.conv3x3(x, blk.up[0], blk.up[1], B, H, W, C, upsample=True, out=cat_dst(C, 4 * H * W))
                H, W = 2 * H, 2 * W
            if stop_up is not None and i == stop_up:
                return x, H, W
        C = x.shape[-1]
        if self.conv_out_n4 is not None:
            x = ops.groupnorm(x, self.norm_out[0], self.norm_out[1], cfg.norm_num_groups, cfg.norm_eps, silu=True)      # plain activations (no pair rows)
            eps = ops.conv3x3_n4(x, self.conv_out_n4, self.conv_out[1], B, H, W, C)
        else:
            x = self._gn(x, self.norm_out, cfg.norm_eps, True)
            eps = ops.conv3x3(x, self.conv_out[0], self.conv_out[1], B, H, W, C, out_f32=True)
        eps = ops.nhwc_to_nchw_f32(eps, cfg.out_channels, H, W)
        self._in_phase_a = False
        if B != BB:                                           # dropped tail / stored K / V: the reference rows' eps is not computed (zeros)
            eps = torch.zeros(BB, *eps.shape[1:], dtype=eps.dtype, device=eps.device).index_copy_(0, ru["idx_a"], eps)
        return eps
