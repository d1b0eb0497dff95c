"""LoRA adapters (PEFT-compatible) on the fused projections of the decoder.

Adapters are stored per HF target module (q_proj, k_proj, ..., down_proj) so PEFT checkpoints map
1:1; at run time the adapters of one fused projection form a :class:`ops.LoRAGroup` and are
executed inside the projection's MFMA GEMM. This is the "Transfer Learning (LoRA/PEFT)" stage the
reference README declares (README.md:15,29) but does not implement.
"""
from __future__ import annotations

import contextlib
import json
import math
import os
from dataclasses import asdict, dataclass, field
from typing import Dict, List, Optional

import torch
import torch.nn as nn

from .. import ops

# projection name -> (fused group, row offset function)
_LLAMA_GROUPS = {
    "q_proj": "qkv", "k_proj": "qkv", "v_proj": "qkv", "o_proj": "o",
    "gate_proj": "gate_up", "up_proj": "gate_up", "down_proj": "down",
}
_OPT_GROUPS = {"q_proj": "qkv", "k_proj": "qkv", "v_proj": "qkv", "out_proj": "o", "fc1": "fc1", "fc2": "fc2"}


@dataclass
class LoraConfig:
    r: int = 16
    lora_alpha: float = 32.0
    lora_dropout: float = 0.0
    target_modules: List[str] = field(default_factory=lambda: ["q_proj", "v_proj"])
    bias: str = "none"
    task_type: str = "CAUSAL_LM"
    peft_type: str = "LORA"
    base_model_name_or_path: str = ""
    fan_in_fan_out: bool = False
    inference_mode: bool = False
    init_lora_weights: bool = True
    modules_to_save: Optional[List[str]] = None
    layers_to_transform: Optional[List[int]] = None
    use_rslora: bool = False

    @property
    def scaling(self) -> float:
        return self.lora_alpha / (math.sqrt(self.r) if self.use_rslora else self.r)

    def to_json(self) -> dict:
        d = asdict(self)
        d["target_modules"] = sorted(self.target_modules)
        return d


def _proj_rows(cfg, proj: str):
    """(row offset, rows) of an HF projection inside its fused weight."""
    Hq, Hkv, D, F, H = cfg.num_heads, cfg.num_kv_heads, cfg.head_dim, cfg.intermediate_size, cfg.hidden_size
    table = {
        "q_proj": (0, Hq * D), "k_proj": (Hq * D, Hkv * D), "v_proj": ((Hq + Hkv) * D, Hkv * D),
        "o_proj": (0, H), "out_proj": (0, H), "gate_proj": (0, F), "up_proj": (F, F), "down_proj": (0, H),
        "fc1": (0, F), "fc2": (0, H),
    }
    return table[proj]


def _proj_in(cfg, proj: str) -> int:
    if proj in ("o_proj", "out_proj"):
        return cfg.num_heads * cfg.head_dim
    if proj in ("down_proj", "fc2"):
        return cfg.intermediate_size
    return cfg.hidden_size


def group_map(cfg) -> Dict[str, str]:
    return _OPT_GROUPS if cfg.arch == "opt" else _LLAMA_GROUPS


def _group_out(cfg, group: str) -> int:
    return {"qkv": cfg.qkv_dim, "o": cfg.hidden_size, "gate_up": 2 * cfg.intermediate_size,
            "down": cfg.hidden_size, "fc1": cfg.intermediate_size, "fc2": cfg.hidden_size}[group]


def attach_lora(model, r=16, alpha=32.0, targets=None, dropout=0.0, seed=0):
    cfg = model.cfg
    gm = group_map(cfg)
    if targets is None or targets == "all":
        targets = list(gm.keys())
    targets = [t for t in targets if t in gm]
    if not 0.0 <= dropout < 1.0:
        raise ValueError(f"lora_dropout must be in [0, 1), got {dropout}")
    lcfg = LoraConfig(r=r, lora_alpha=alpha, lora_dropout=dropout, target_modules=list(targets),
                      base_model_name_or_path=cfg.name)
    g = torch.Generator(device="cpu").manual_seed(seed)
    dev = model.embed.device
    for layer in model.layers:
        layer.lora = {}
        layer.lora_params = nn.ParameterDict()
        groups: Dict[str, list] = {}
        for proj in targets:
            groups.setdefault(gm[proj], []).append(proj)
        for grp, projs in groups.items():
            a_list, b_list, c0s, scales = [], [], [], []
            for proj in projs:
                k_in = _proj_in(cfg, proj)
                row0, n = _proj_rows(cfg, proj)
                a = torch.empty(r, k_in)
                # PEFT init: A ~ kaiming_uniform(a=sqrt(5)), B = 0
                bound = 1.0 / math.sqrt(k_in)
                a.uniform_(-bound, bound, generator=g)
                pa = nn.Parameter(a.to(dev))
                pb = nn.Parameter(torch.zeros(n, r, device=dev))
                layer.lora_params[f"{proj}_A"] = pa
                layer.lora_params[f"{proj}_B"] = pb
                a_list.append(pa)
                b_list.append(pb)
                c0s.append(row0)
                scales.append(lcfg.scaling)
            layer.lora[grp] = ops.LoRAGroup(projs, a_list, b_list, c0s, scales, _group_out(cfg, grp),
                                            dropout=float(dropout))
    model.lora_config = lcfg
    model.refresh_lora()
    return lcfg


def _layer_prefix(cfg, i):
    return f"base_model.model.model.decoder.layers.{i}" if cfg.arch == "opt" else f"base_model.model.model.layers.{i}"


def _module_path(cfg, proj):
    if cfg.arch == "opt":
        return f"self_attn.{proj}" if proj in ("q_proj", "k_proj", "v_proj", "out_proj") else proj
    return f"self_attn.{proj}" if proj in ("q_proj", "k_proj", "v_proj", "o_proj") else f"mlp.{proj}"


def adapter_state_dict(model) -> Dict[str, torch.Tensor]:
    """PEFT key layout: base_model.model.model.layers.{i}.self_attn.q_proj.lora_A.weight [r, in]."""
    cfg = model.cfg
    out = {}
    for i, layer in enumerate(model.layers):
        for key, p in layer.lora_params.items():
            proj, ab = key.rsplit("_", 1)
            name = f"{_layer_prefix(cfg, i)}.{_module_path(cfg, proj)}.lora_{ab}.weight"
            out[name] = p.detach().float().cpu().contiguous()
    return out


def save_adapter(model, path: str):
    from safetensors.torch import save_file

    os.makedirs(path, exist_ok=True)
    save_file(adapter_state_dict(model), os.path.join(path, "adapter_model.safetensors"), metadata={"format": "pt"})
    with open(os.path.join(path, "adapter_config.json"), "w") as f:
        json.dump(model.lora_config.to_json(), f, indent=2)


def load_adapter(model, path: str):
    from safetensors.torch import load_file

    with open(os.path.join(path, "adapter_config.json")) as f:
        d = json.load(f)
    lc = LoraConfig(**{k: v for k, v in d.items() if k in LoraConfig.__dataclass_fields__})
    if not hasattr(model, "lora_config") or model.lora_config.r != lc.r or \
            sorted(model.lora_config.target_modules) != sorted(lc.target_modules):
        attach_lora(model, lc.r, lc.lora_alpha, lc.target_modules, lc.lora_dropout)
    sd = load_file(os.path.join(path, "adapter_model.safetensors"))
    cfg = model.cfg
    with torch.no_grad():
        for i, layer in enumerate(model.layers):
            for key, p in layer.lora_params.items():
                proj, ab = key.rsplit("_", 1)
                name = f"{_layer_prefix(cfg, i)}.{_module_path(cfg, proj)}.lora_{ab}.weight"
                p.copy_(sd[name].to(p.device, p.dtype))
    model.lora_config = lc
    model.refresh_lora()
    return lc


@torch.no_grad()
def merge_lora(model, sign: float = 1.0):
    """W += sign * s * B A for every adapter (sign=-1 unmerges). Used to export a merged HF model."""
    cfg = model.cfg
    for layer in model.layers:
        for grp_name, grp in layer.lora.items():
            w = _group_weight(layer, cfg, grp_name)
            for a, b, c0, s in zip(grp.a, grp.b, grp.col0, grp.scale):
                delta = (b.float() @ a.float()) * s * sign
                w[c0:c0 + b.shape[0]] += delta.to(w.dtype)


@torch.no_grad()
def merge_and_drop_lora(model):
    """Fold every adapter into its base weight (W += s B A) and remove the adapters, leaving a plain
    model (full fine-tuning after a LoRA stage, merged export)."""
    if getattr(model, "lora_config", None) is None:
        return
    merge_lora(model)
    for layer in model.layers:
        layer.lora = {}
        layer.lora_params = nn.ParameterDict()
    del model.lora_config


def _group_weight(layer, cfg, grp):
    return {"qkv": layer.qkv_w, "o": layer.o_w, "gate_up": getattr(layer, "gate_up_w", None),
            "down": getattr(layer, "down_w", None), "fc1": getattr(layer, "fc1_w", None),
            "fc2": getattr(layer, "fc2_w", None)}[grp]


# ------------------------------------------------------------------------------------------------
# Per-request adapters: several adapters resident over one frozen base (docs/DESIGN.md "Per-request
# adapters")
_BANK_GROUPS = (("qkv", ("q_proj", "k_proj", "v_proj"), "ln1_w"), ("o", ("o_proj",), None),
                ("gate_up", ("gate_proj", "up_proj"), "ln2_w"), ("down", ("down_proj",), None))


class AdapterBank:
    """``slots`` LoRA adapters of rank <= ``r_max`` resident over one frozen Llama / Mistral base, for
    decode steps whose rows each pick their own adapter (``ContinuousBatcher(adapters=bank)``).

    Per layer and fused projection (qkv, o, gate_up, down) the bank holds, for all slots at fixed
    addresses (``load`` / ``unload`` write in place, so captured decode steps stay valid):
      * ``a_img`` [slots, nseg R, K] bf16: ``s A`` of every sub-projection, times the RMSNorm weight
        where the decode step folds it into the base weight (qkv, gate_up), rounded to bf16 once;
      * ``b_img`` [slots, N, R] bf16: per output column the R entries of its own sub-projection;
      * for the folded projections ``a_raw`` (``s A`` without the norm weight) for the token-parallel
        path, which applies the norm as its own kernel.
    Ranks below R are zero-padded, a target module an adapter lacks is zeros. The token-parallel
    path (prefill, scoring) runs ONE slot through the K-extension GEMMs: :meth:`active` points
    every projection's ``ops.LoRAGroup`` compute images at that slot, unmerged."""

    def __init__(self, model, slots: int = 8, r_max: int = 16):
        cfg = model.cfg
        if cfg.arch == "opt":
            raise ValueError("AdapterBank: learned-position (opt) models have no fused decode layer")
        if r_max not in (8, 16, 32, 64):
            raise ValueError(f"AdapterBank: r_max must be 8, 16, 32 or 64, got {r_max}")
        if slots < 1:
            raise ValueError("AdapterBank: at least one slot")
        self.model, self.cfg, self.slots, self.R = model, cfg, int(slots), int(r_max)
        self.names: List[Optional[str]] = [None] * self.slots
        self.version = [0] * self.slots
        dev, dt = model.embed.device, model.dtype
        R = self.R
        self.layers = []   # per layer: group -> dict(a_img, b_img, a_raw, segs, scratch LoRAGroup)
        self._master = {}  # slot -> {(layer, group): fp32 s A on the CPU} of the folded projections
        self._fold_key = {}
        for layer in model.layers:
            ent = {}
            for grp, projs, _ in _BANK_GROUPS:
                K = _proj_in(cfg, projs[0])
                N = _group_out(cfg, grp)
                nseg = len(projs)
                a_img = torch.zeros(self.slots, nseg * R, K, dtype=dt, device=dev)
                folded = grp in ("qkv", "gate_up")
                rp = max(64, (nseg * R + 63) // 64 * 64)
                # the one-slot K-extension images of the token-parallel path; the off-diagonal blocks
                # and the padding of ub / a_pad stay zero, a slot switch copies the diagonal blocks
                g = ops.LoRAGroup(list(projs), [], [], [_proj_rows(cfg, p)[0] for p in projs], [1.0] * nseg, N)
                g.a_pad = torch.zeros(rp, K, dtype=dt, device=dev)
                g.ub = torch.zeros(N, rp, dtype=dt, device=dev)
                ent[grp] = dict(a_img=a_img, b_img=torch.zeros(self.slots, N, R, dtype=dt, device=dev),
                                a_raw=torch.zeros_like(a_img) if folded else a_img,
                                segs=tuple(_proj_rows(cfg, p)[0] for p in projs[1:]), group=g)
            self.layers.append(ent)
        self._pf_slot = None  # (slot, version) the one-slot images hold

    # -------------------------------------------------------------- slots
    def loaded(self) -> List[str]:
        return [n for n in self.names if n is not None]

    def slot(self, name: Optional[str]) -> int:
        """Slot of a loaded adapter; -1 for None (the base model)."""
        if name is None:
            return -1
        if name not in self.names:
            raise KeyError(f"adapter {name!r} is not loaded (loaded: {self.loaded()})")
        return self.names.index(name)

    def layer(self, li: int):
        return self.layers[li]

    @torch.no_grad()
    def load(self, name: str, peft_dir: str) -> int:
        """Read a PEFT adapter directory (``save_adapter``'s layout) into ``name``'s slot — a free one,
        or in place over the adapter of that name. Everything is validated before a byte is written."""
        from safetensors.torch import load_file

        if not isinstance(name, str) or not name:
            raise ValueError("AdapterBank.load: the adapter name must be a non-empty string")
        with open(os.path.join(peft_dir, "adapter_config.json")) as f:
            d = json.load(f)
        lc = LoraConfig(**{k: v for k, v in d.items() if k in LoraConfig.__dataclass_fields__})
        if lc.r > self.R:
            raise ValueError(f"adapter {name!r}: rank {lc.r} exceeds the bank's r_max {self.R}")
        sd = load_file(os.path.join(peft_dir, "adapter_model.safetensors"))
        cfg, R, s = self.cfg, self.R, float(lc.scaling)
        staged, used = [], set()
        for li in range(len(self.layers)):
            for grp, projs, _ in _BANK_GROUPS:
                K, N = _proj_in(cfg, projs[0]), _group_out(cfg, grp)
                a = torch.zeros(len(projs) * R, K)
                b = torch.zeros(N, R)
                for i, proj in enumerate(projs):
                    base = f"{_layer_prefix(cfg, li)}.{_module_path(cfg, proj)}"
                    ka, kb = f"{base}.lora_A.weight", f"{base}.lora_B.weight"
                    if ka not in sd and kb not in sd:
                        continue  # a target module this adapter lacks: zeros
                    if ka not in sd or kb not in sd:
                        raise ValueError(f"adapter {name!r}: {base} has only one of lora_A / lora_B")
                    row0, n = _proj_rows(cfg, proj)
                    A, B = sd[ka].float(), sd[kb].float()
                    if A.dim() != 2 or B.dim() != 2 or A.shape[1] != K or B.shape[0] != n or A.shape[0] != B.shape[1] \
                            or A.shape[0] > R:
                        raise ValueError(f"adapter {name!r}: {base} has A {tuple(A.shape)}, B {tuple(B.shape)}; the base "
                                         f"model needs A [r <= {R}, {K}], B [{n}, r]")
                    r = A.shape[0]
                    a[i * R:i * R + r] = A * s
                    b[row0:row0 + n, :r] = B
                    used.update((ka, kb))
                staged.append((li, grp, a, b))
        extra = [k for k in sd if k not in used]
        if extra:
            raise ValueError(f"adapter {name!r}: {len(extra)} tensors do not belong to this base model (e.g. {extra[0]})")
        if name in self.names:
            sl = self.names.index(name)
        elif None in self.names:
            sl = self.names.index(None)
        else:
            raise ValueError(f"AdapterBank: all {self.slots} slots are taken ({self.loaded()}); unload one first")
        master = {}
        for li, grp, a, b in staged:
            e = self.layers[li][grp]
            e["b_img"][sl].copy_(b)
            e["a_raw"][sl].copy_(a)
            if e["a_raw"] is not e["a_img"]:
                master[(li, grp)] = a
        self.refresh()  # the other slots' folds and the recorded norm-weight keys are current first
        self._master[sl] = master
        self.names[sl] = name
        self.version[sl] += 1
        self._fold(sl)
        return sl

    @torch.no_grad()
    def unload(self, name: str):
        sl = self.slot(name)
        for ent in self.layers:
            for e in ent.values():
                e["a_img"][sl].zero_()
                e["b_img"][sl].zero_()
                e["a_raw"][sl].zero_()
        self._master.pop(sl, None)
        self.names[sl] = None
        self.version[sl] += 1

    @torch.no_grad()
    def _fold(self, sl: int, li: Optional[int] = None):
        """a_img of the folded projections (of layer ``li``, or all) = bf16(s A diag(norm weight)) from
        the fp32 master and the layer's current norm weight."""
        for (l2, grp), a in self._master.get(sl, {}).items():
            if li is None or l2 == li:
                nw = getattr(self.model.layers[l2], "ln1_w" if grp == "qkv" else "ln2_w")
                self.layers[l2][grp]["a_img"][sl].copy_(a * nw.detach().float().cpu()[None, :])

    @torch.no_grad()
    def refresh(self):
        """Rebuild the folded a_img of every slot for each layer whose norm weights are not the ones
        of its last fold (data pointer or in-place version: a checkpoint load, an optimizer step).
        ``load`` and the batcher call it; call it after changing norm weights under a running batcher."""
        for li, layer in enumerate(self.model.layers):
            key = (layer.ln1_w.data_ptr(), layer.ln1_w._version, layer.ln2_w.data_ptr(), layer.ln2_w._version)
            if self._fold_key.get(li) != key:
                for sl in self._master:
                    self._fold(sl, li)
                self._fold_key[li] = key

    # -------------------------------------------------------------- token-parallel path: one slot
    @contextlib.contextmanager
    def active(self, name: Optional[str]):
        """Run the model's token-parallel forwards (prefill, scoring) with adapter ``name`` unmerged
        — the K-extension GEMMs over this slot's images — or, for None, as the base model."""
        sl = self.slot(name)
        layers = self.model.layers
        saved = [(layer.lora, layer.lora_enabled) for layer in layers]
        if sl >= 0 and self._pf_slot != (sl, self.version[sl]):
            R = self.R
            with torch.no_grad():
                for ent in self.layers:
                    for e in ent.values():
                        g = e["group"]
                        nr = e["a_raw"].shape[1]
                        g.merged_dirty = True  # a merged copy of another slot must never be reused
                        g.a_pad[:nr].copy_(e["a_raw"][sl])
                        bounds = list(g.col0) + [g.n_out]
                        for i in range(len(g.col0)):
                            g.ub[bounds[i]:bounds[i + 1], i * R:(i + 1) * R].copy_(e["b_img"][sl, bounds[i]:bounds[i + 1]])
            self._pf_slot = (sl, self.version[sl])
        try:
            for layer, ent in zip(layers, self.layers):
                layer.lora = {grp: e["group"] for grp, e in ent.items()} if sl >= 0 else {}
                layer.lora_enabled = True
            yield
        finally:
            for layer, (lo, en) in zip(layers, saved):
                layer.lora, layer.lora_enabled = lo, en
