"""Rank bodies for the multi-process CPU (gloo) tests. Module-level so `spawn` can pickle them."""
import os

import torch


def tiny_llama(seed=0, **kw):
    from shuffle_exchange_amd.models import LlamaForCausalLM, llama_config
    torch.manual_seed(seed)
    cfg = llama_config("llama-tiny", **kw)
    return LlamaForCausalLM(cfg), cfg


def global_batches(cfg, world, mbs, seq, steps, seed=1):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, cfg.vocab_size, (world * mbs, seq), generator=g) for _ in range(steps)]


def full_params(engine):
    """Full (gathered) parameters by name, on CPU, fp32."""
    if engine.zero_optimization_stage() == 3:
        sd = engine._zero3_consolidated_16bit_state_dict()
        return {k: v.float() for k, v in sd.items() if k in dict(engine.module.named_parameters())}
    return {n: p.detach().float().clone() for n, p in engine.module.named_parameters()}


def case_train(rank, world, ds_config, steps, mbs, seq, se_kwargs=None, seed=0):
    import shuffle_exchange_amd as sxe
    model, cfg = tiny_llama(seed)
    eng, _, _, _ = sxe.initialize(model=model, config=ds_config, **(se_kwargs or {}))
    batches = global_batches(cfg, world, mbs, seq, steps)
    losses = []
    for b in batches:
        local = b[rank * mbs:(rank + 1) * mbs]
        loss = eng(local, labels=local)
        eng.backward(loss)
        eng.step()
        losses.append(float(loss.detach()))
    return {"params": full_params(eng), "losses": losses}


class _PlainLion(torch.optim.Optimizer):
    """Lion from the formula in the header comment of csrc/kernels/optim.hip, in the parameters' own
    dtype: u = sign(b1*m + (1-b1)*g); p -= lr*(u + wd*p); m = b2*m + (1-b2)*g."""

    def __init__(self, params, lr=1e-4, betas=(0.9, 0.99), weight_decay=0.0):
        super().__init__(params, dict(lr=lr, betas=betas, weight_decay=weight_decay))

    @torch.no_grad()
    def step(self):
        for group in self.param_groups:
            b1, b2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if not st:
                    st["exp_avg"] = torch.zeros_like(p)
                m, g = st["exp_avg"], p.grad
                u = (b1 * m + (1 - b1) * g).sign()
                p.sub_(group["lr"] * (u + group["weight_decay"] * p))
                m.mul_(b2).add_(g, alpha=1 - b2)


def reference_train(ds_opt, steps, world, mbs, seq, seed=0, clip=0.0, dtype=None):
    """Single-process reference on the global batch with torch.optim (Lion: _PlainLion). ``dtype``
    (e.g. torch.float64) converts the model first, to measure what fp32 rounding alone moves."""
    model, cfg = tiny_llama(seed)
    if dtype is not None:
        model = model.to(dtype)
    p = ds_opt["params"]
    kind = ds_opt["type"].lower()
    if kind in ("adamw", "adam"):
        opt = torch.optim.AdamW(model.parameters(), lr=p["lr"], weight_decay=p.get("weight_decay", 0.0),
                                betas=tuple(p.get("betas", (0.9, 0.999))), eps=p.get("eps", 1e-8))
    elif kind == "adagrad":
        opt = torch.optim.Adagrad(model.parameters(), lr=p["lr"], eps=p.get("eps", 1e-10),
                                  weight_decay=p.get("weight_decay", 0.0))
    elif kind == "lion":
        opt = _PlainLion(model.parameters(), lr=p["lr"], betas=tuple(p.get("betas", (0.9, 0.99))),
                         weight_decay=p.get("weight_decay", 0.0))
    elif kind == "sgd":
        opt = torch.optim.SGD(model.parameters(), lr=p["lr"])
    else:
        raise ValueError(f"reference_train: no reference optimizer for type {ds_opt['type']!r}")
    for b in global_batches(cfg, world, mbs, seq, steps):
        loss = model(b, labels=b)
        opt.zero_grad()
        loss.backward()
        if clip:
            torch.nn.utils.clip_grad_norm_(model.parameters(), clip)
        opt.step()
    return {n: q.detach().float().clone() for n, q in model.named_parameters()}


def case_shuffle_groups(rank, world, slice_count, rings, shuffle_step, calls):
    import shuffle_exchange_amd as sxe
    model, cfg = tiny_llama(0)
    ds = {"train_micro_batch_size_per_gpu": 1, "zero_optimization": {"stage": 2},
          "optimizer": {"type": "SGD", "params": {"lr": 0.1}}}
    eng, _, _, _ = sxe.initialize(model=model, config=ds, method="shuffle", slice_count=slice_count, rings=rings,
                                  shuffle_step=shuffle_step)
    hist = [list(eng.optimizer.se.current_groups())]
    for _ in range(calls):
        eng.shuffle_exchange()
        hist.append(list(eng.optimizer.se.current_groups()))
    return hist


def case_gossip(rank, world, steps):
    import shuffle_exchange_amd as sxe
    from shuffle_exchange_amd import comm
    model, cfg = tiny_llama(0)
    ds = {"train_micro_batch_size_per_gpu": 1, "zero_optimization": {"stage": 1},
          "optimizer": {"type": "SGD", "params": {"lr": 0.05}}}
    eng, _, _, _ = sxe.initialize(model=model, config=ds, method="Gossip", slice_count=1)
    batches = global_batches(cfg, world, 1, 16, steps)
    for b in batches:
        local = b[rank:rank + 1]
        loss = eng(local, labels=local)
        eng.backward(loss)
        eng.step()
    se = eng.optimizer.se
    # pending (queued) mass counts as well: alpha is conserved over alpha + queued messages
    mass = float(se.alpha) + sum(float(a) for a, _ in se.queue)
    t = torch.tensor([mass])
    comm.all_reduce(t)
    eng.synchronization()
    return {"mass": float(t), "params": full_params(eng)}


def case_ckpt(rank, world, stage, tmpdir, steps_a, steps_b):
    import shuffle_exchange_amd as sxe
    from shuffle_exchange_amd import comm
    ds = {"train_micro_batch_size_per_gpu": 2, "zero_optimization": {"stage": stage},
          "optimizer": {"type": "AdamW", "params": {"lr": 5e-3}},
          "scheduler": {"type": "WarmupLR", "params": {"warmup_num_steps": 3, "warmup_max_lr": 5e-3}}}
    model, cfg = tiny_llama(0)
    eng, _, _, _ = sxe.initialize(model=model, config=ds)
    batches = global_batches(cfg, world, 2, 16, steps_a + steps_b)

    def run(e, bs):
        out = []
        for b in bs:
            local = b[rank * 2:(rank + 1) * 2]
            loss = e(local, labels=local)
            e.backward(loss)
            e.step()
            out.append(float(loss.detach()))
        return out

    run(eng, batches[:steps_a])
    eng.save_checkpoint(tmpdir, client_state={"marker": 7})
    cont = run(eng, batches[steps_a:])
    model2, _ = tiny_llama(123)  # different init: everything must come from the checkpoint
    eng2, _, _, _ = sxe.initialize(model=model2, config=ds)
    path, client = eng2.load_checkpoint(tmpdir)
    resumed = run(eng2, batches[steps_a:])
    files = sorted(os.listdir(os.path.join(tmpdir, f"global_step{steps_a}")))
    return {"cont": cont, "resumed": resumed, "client": client.get("marker"), "files": files,
            "lr": eng2.get_lr()[0], "lr_ref": eng.get_lr()[0]}


def case_collectives(rank, world):
    from shuffle_exchange_amd import comm
    comm.enable_fingerprint(True)
    comm.reset_fingerprint()
    x = torch.full((8,), float(rank + 1))
    comm.all_reduce(x)
    out = torch.empty(world * 4)
    comm.all_gather_into_tensor(out, torch.full((4,), float(rank)))
    rs = torch.empty(2)
    comm.reduce_scatter_tensor(rs, torch.arange(world * 2, dtype=torch.float32))
    a2a = torch.empty(world)
    comm.all_to_all_single(a2a, torch.full((world,), float(rank)))
    ok = comm.verify_fingerprints()
    return {"ar": x.tolist(), "ag": out.tolist(), "rs": rs.tolist(), "a2a": a2a.tolist(), "fp_ok": ok}


def case_fingerprint_mismatch(rank, world):
    from shuffle_exchange_amd import comm
    comm.enable_fingerprint(True)
    comm.reset_fingerprint()
    x = torch.ones(4 if rank == 0 else 8)
    from shuffle_exchange_amd.comm import comm as comm_impl
    comm_impl._fp("all_reduce", None, x)  # record a divergent collective without running it
    try:
        comm.verify_fingerprints()
        return "no-error"
    except RuntimeError:
        return "mismatch-detected"


# ------------------------------------------------------------------------------------------- MoE
def _moe_global(seed=0):
    from shuffle_exchange_amd.moe import MoE
    torch.manual_seed(seed)
    m = MoE(32, None, num_experts=4, ep_size=1, k=2, capacity_factor=4.0, min_capacity=64, use_rts=False,
            top2_2nd_expert_sampling=False, intermediate_size=48)
    return m


def moe_single_reference():
    from shuffle_exchange_amd.parallel import groups
    groups.reset()
    m = _moe_global()
    m._groups_ready = True
    torch.manual_seed(3)
    x = torch.randn(2, 2, 8, 32)  # [rank, batch, seq, H]: both ranks' tokens
    outs = []
    for r in range(2):
        o, l, c = m(x[r])
        outs.append(o)
        o.square().sum().backward()
    ex = m.deepspeed_moe.experts
    return {"out": torch.stack(outs), "g_up": ex.w_gate_up.grad.clone(), "g_down": ex.w_down.grad.clone()}


def case_moe_ep(rank, world):
    from shuffle_exchange_amd.moe import MoE
    g = _moe_global()
    torch.manual_seed(0)
    m = MoE(32, None, num_experts=4, ep_size=2, k=2, capacity_factor=4.0, min_capacity=64, use_rts=False,
            top2_2nd_expert_sampling=False, intermediate_size=48)
    with torch.no_grad():
        m.deepspeed_moe.gate.wg.weight.copy_(g.deepspeed_moe.gate.wg.weight)
        ex, gex = m.deepspeed_moe.experts, g.deepspeed_moe.experts
        ex.w_gate_up.copy_(gex.w_gate_up[rank * 2:rank * 2 + 2])
        ex.w_down.copy_(gex.w_down[rank * 2:rank * 2 + 2])
    torch.manual_seed(3)
    x = torch.randn(2, 2, 8, 32)
    outs = []
    o, l, c = m(x[rank])
    o.square().sum().backward()
    # gather every rank's output so each test rank can compare the full picture
    from shuffle_exchange_amd import comm
    full = [torch.empty_like(o) for _ in range(world)]
    comm.all_gather(full, o.detach().contiguous())
    ex = m.deepspeed_moe.experts
    return {"out": torch.stack(full), "g_up": ex.w_gate_up.grad.clone(), "g_down": ex.w_down.grad.clone()}


def case_mixtral_train(rank, world, stage):
    import shuffle_exchange_amd as sxe
    from shuffle_exchange_amd.models.mixtral import MixtralForCausalLM, mixtral_config
    torch.manual_seed(0)
    cfg = mixtral_config("mixtral-tiny", ep_size=2)
    model = MixtralForCausalLM(cfg)
    ds = {"train_micro_batch_size_per_gpu": 2, "zero_optimization": {"stage": stage},
          "optimizer": {"type": "AdamW", "params": {"lr": 3e-3}}, "gradient_clipping": 1.0}
    eng, _, _, _ = sxe.initialize(model=model, config=ds)
    g = torch.Generator().manual_seed(7 + rank)
    ids = torch.randint(0, cfg.vocab_size, (2, 32), generator=g)
    losses = []
    for _ in range(6):
        loss = eng(ids, labels=ids)
        eng.backward(loss)
        eng.step()
        losses.append(float(loss.detach()))
    return {"losses": losses}


def case_zero3_reuse(rank, world, max_reuse, steps, mbs, seq):
    """ZeRO-3 with a reuse-distance budget: count the unit all-gathers issued by the optimizer."""
    import shuffle_exchange_amd as sxe
    model, cfg = tiny_llama(0)
    ds = {"train_micro_batch_size_per_gpu": mbs,
          "zero_optimization": {"stage": 3, "stage3_param_persistence_threshold": 0,
                                "stage3_max_reuse_distance": max_reuse, "stage3_max_live_parameters": 10**12},
          "optimizer": {"type": "AdamW", "params": {"lr": 1e-2, "weight_decay": 0.01}}}
    eng, _, _, _ = sxe.initialize(model=model, config=ds)
    opt = eng.optimizer
    n_gathers = [0]
    orig = opt._launch_gather

    def counting(u):
        n_gathers[0] += 1
        return orig(u)
    opt._launch_gather = counting
    for b in global_batches(cfg, world, mbs, seq, steps):
        local = b[rank * mbs:(rank + 1) * mbs]
        loss = eng(local, labels=local)
        eng.backward(loss)
        eng.step()
    opt._launch_gather = orig
    return {"params": full_params(eng), "gathers": n_gathers[0]}


def case_tied_zero3(rank, world, steps):
    """ZeRO-3 with tied embedding / LM head and no reuse budget: the LM head must fetch the
    embedding's unit itself (external parameter)."""
    import shuffle_exchange_amd as sxe
    model, cfg = tiny_llama(0, tie_word_embeddings=True)
    ds = {"train_micro_batch_size_per_gpu": 1,
          "zero_optimization": {"stage": 3, "stage3_param_persistence_threshold": 0, "stage3_max_reuse_distance": 0},
          "optimizer": {"type": "SGD", "params": {"lr": 0.1}}}
    eng, _, _, _ = sxe.initialize(model=model, config=ds)
    for b in global_batches(cfg, world, 1, 16, steps):
        local = b[rank:rank + 1]
        loss = eng(local, labels=local)
        eng.backward(loss)
        eng.step()
    return {"params": full_params(eng), "fgs": [fg.name for fg in eng.optimizer.fgroups]}


def case_zero3_defer(rank, world, defer, steps, mbs, gas, seq, retain=False):
    """ZeRO-3 with gradient accumulation, with/without the deferred (boundary-only) reduce-scatter;
    counts the reduce-scatters issued."""
    import shuffle_exchange_amd as sxe
    from shuffle_exchange_amd import comm as dist
    model, cfg = tiny_llama(0)
    ds = {"train_micro_batch_size_per_gpu": mbs, "gradient_accumulation_steps": gas,
          "zero_optimization": {"stage": 3, "stage3_param_persistence_threshold": 0, "stage3_defer_reduce": defer,
                                "stage3_retain_params_in_step": retain},
          "optimizer": {"type": "AdamW", "params": {"lr": 1e-2, "weight_decay": 0.01}}}
    eng, _, _, _ = sxe.initialize(model=model, config=ds)
    opt = eng.optimizer
    n_ag = [0]
    orig_gather = opt._launch_gather

    def counting_gather(u):
        n_ag[0] += 1
        return orig_gather(u)
    opt._launch_gather = counting_gather
    n_rs = [0]
    orig = dist.reduce_scatter_tensor

    def counting(*a, **k):
        n_rs[0] += 1
        return orig(*a, **k)
    dist.reduce_scatter_tensor = counting
    import shuffle_exchange_amd.runtime.zero.stage3 as s3
    s3_orig = s3.dist.reduce_scatter_tensor
    s3.dist.reduce_scatter_tensor = counting
    try:
        for b in global_batches(cfg, world, mbs, seq, steps * gas):
            local = b[rank * mbs:(rank + 1) * mbs]
            loss = eng(local, labels=local)
            eng.backward(loss)
            eng.step()
    finally:
        dist.reduce_scatter_tensor = orig
        s3.dist.reduce_scatter_tensor = s3_orig
    opt._launch_gather = orig_gather
    return {"params": full_params(eng), "rs": n_rs[0], "ag": n_ag[0], "defer": eng.optimizer.defer_reduce,
            "n_units": sum(len(us) for us in opt.units)}


def case_zero_init(rank, world, layers, steps):
    """zero.Init partitions at construction (different RNG per rank), ZeRO-3 trains from it."""
    import shuffle_exchange_amd as sxe
    from shuffle_exchange_amd.models import LlamaForCausalLM, llama_config
    torch.manual_seed(100 + rank)  # deliberately different per rank
    cfg = llama_config("llama-tiny", num_hidden_layers=layers)
    init = sxe.zero.Init(dtype=torch.float32)
    with init:
        model = LlamaForCausalLM(cfg)
    empty = all(p.data.numel() == 0 for p in model.parameters())
    full_numel = cfg.num_params()
    layer_numel = sum(p.ds_numel for p in model.layers[0].parameters())
    emb_numel = model.embed_tokens.weight.ds_numel
    # whole-tensor edit between construction and initialize(): rank 0's value must win everywhere
    w = model.norm.weight
    with sxe.zero.GatheredParameters([w], modifier_rank=0):
        w.data.fill_(1.5 if rank == 0 else -7.0)
    ds = {"train_micro_batch_size_per_gpu": 1, "zero_optimization": {"stage": 3, "stage3_param_persistence_threshold": 0},
          "optimizer": {"type": "AdamW", "params": {"lr": 1e-2}}}
    eng, _, _, _ = sxe.initialize(model=model, config=ds)
    left = sum(1 for p in model.parameters() if hasattr(p, "ds_tensor"))
    before = full_params(eng)
    g = torch.Generator().manual_seed(7)
    losses = []
    for _ in range(steps):
        b = torch.randint(0, cfg.vocab_size, (world, 16), generator=g)[rank:rank + 1]
        loss = eng(b, labels=b)
        eng.backward(loss)
        eng.step()
        losses.append(float(loss.detach()))
    return {"stats": dict(init.stats), "empty": empty, "full_numel": full_numel, "layer_numel": layer_numel,
            "emb_numel": emb_numel, "left": left, "before": before, "after": full_params(eng), "losses": losses}


def case_broadcast_coalesced(rank, world):
    from shuffle_exchange_amd.runtime.engine import broadcast_coalesced
    torch.manual_seed(rank)
    ts = [torch.randn(1000), torch.randn(10), torch.randn(300, 3).t(), torch.randn(5000).double(), torch.randn(7)]
    n = broadcast_coalesced(ts, 0, None, bucket_bytes=4096)
    torch.manual_seed(0)
    ref = [torch.randn(1000), torch.randn(10), torch.randn(300, 3).t(), torch.randn(5000).double(), torch.randn(7)]
    return {"ok": all(torch.equal(a, b) for a, b in zip(ts, ref)), "n": n}


def case_step_meta(rank, world, stage, se_kwargs, steps):
    """Count the collectives of the optimizer step: one fused step-metadata all-reduce per step."""
    import shuffle_exchange_amd as sxe
    from shuffle_exchange_amd import comm
    model, cfg = tiny_llama(0)
    ds = {"train_micro_batch_size_per_gpu": 1, "gradient_clipping": 1.0,
          "zero_optimization": {"stage": stage, "stage3_param_persistence_threshold": 0},
          "optimizer": {"type": "AdamW", "params": {"lr": 1e-2}}}
    eng, _, _, _ = sxe.initialize(model=model, config=ds, **(se_kwargs or {}))
    b = torch.randint(0, cfg.vocab_size, (1, 16), generator=torch.Generator().manual_seed(rank))
    comm.reset_comms_stats()
    for _ in range(steps):
        loss = eng(b, labels=b)
        eng.backward(loss)
        eng.step()
    return comm.get_op_counts()


def case_mixtral_dense_sync(rank, world):
    """ZeRO-0 + expert parallelism with clipping: dense weights stay identical across ranks."""
    import shuffle_exchange_amd as sxe
    from shuffle_exchange_amd.models.mixtral import MixtralForCausalLM, mixtral_config
    torch.manual_seed(0)
    cfg = mixtral_config("mixtral-tiny", ep_size=2)
    model = MixtralForCausalLM(cfg)
    ds = {"train_micro_batch_size_per_gpu": 2, "zero_optimization": {"stage": 0},
          "optimizer": {"type": "AdamW", "params": {"lr": 3e-3}}, "gradient_clipping": 0.01}
    eng, _, _, _ = sxe.initialize(model=model, config=ds)
    ids = torch.randint(0, cfg.vocab_size, (2, 32), generator=torch.Generator().manual_seed(7 + rank))
    for _ in range(3):
        loss = eng(ids, labels=ids)
        eng.backward(loss)
        eng.step()
    from shuffle_exchange_amd.moe.utils import is_moe_param
    return {n: p.detach().float().clone() for n, p in model.named_parameters() if not is_moe_param(p)}


def case_zero3_comm_design(rank, world, steps):
    """ZeRO-3 communicator layout and the post-step refresh collective count."""
    import shuffle_exchange_amd as sxe
    from shuffle_exchange_amd import comm
    model, cfg = tiny_llama(0)
    ds = {"train_micro_batch_size_per_gpu": 1, "zero_optimization": {"stage": 3},
          "optimizer": {"type": "SGD", "params": {"lr": 0.1}}}
    eng, _, _, _ = sxe.initialize(model=model, config=ds)
    opt = eng.optimizer
    n_persist = sum(1 for us in opt.units for u in us if u.persistent)
    refresh = []
    real = opt._refresh_persistent

    def counted():
        comm.reset_comms_stats()
        real()
        refresh.append(sum(n for k, (n, _) in comm.get_comm_volume().items() if "all_gather" in k))
    opt._refresh_persistent = counted
    for b in global_batches(cfg, world, 1, 16, steps):
        local = b[rank:rank + 1]
        loss = eng(local, labels=local)
        eng.backward(loss)
        eng.step()
    return {"same_group": opt.reduce_group is opt.topo.slice_group,
            "rs_ranks": comm.group_ranks(opt.reduce_group), "ag_ranks": comm.group_ranks(opt.topo.slice_group),
            "n_persist": n_persist, "refresh": refresh, "params": full_params(eng)}


def _freeze_lora_style(model):
    """Freeze every MLP projection and the token embedding (a LoRA-style frozen base); attention
    projections, norms and the LM head stay trainable."""
    names = []
    for n, p in model.named_parameters():
        if ".mlp." in n or n.startswith("embed_tokens"):
            p.requires_grad_(False)
            names.append(n)
    return names


def case_zero3_frozen(rank, world, steps, quant, tmpdir, offload=False):
    """zero.Init + ZeRO-3 with frozen base weights: the frozen parameters become gather-only units
    (1/W shard per rank, optionally int8), the forward/backward read them, the trainable ones update."""
    import shuffle_exchange_amd as sxe
    from shuffle_exchange_amd.models import LlamaForCausalLM, llama_config
    torch.manual_seed(5)
    cfg = llama_config("llama-tiny")
    with sxe.zero.Init(dtype=torch.float32):
        model = LlamaForCausalLM(cfg)
    frozen_names = _freeze_lora_style(model)
    ds = {"train_micro_batch_size_per_gpu": 1,
          "zero_optimization": {"stage": 3, "stage3_param_persistence_threshold": 0,
                                "stage3_gather_16bit_weights_on_model_save": True,
                                "zero_quantized_nontrainable_weights": bool(quant)},
          "optimizer": {"type": "AdamW", "params": {"lr": 1e-2, "weight_decay": 0.0}}}
    if offload:  # ZeRO-Infinity: host optimizer + host-resident parameter shards (frozen ones too)
        ds["zero_optimization"]["offload_optimizer"] = {"device": "cpu"}
        ds["zero_optimization"]["offload_param"] = {"device": "cpu"}
    eng, _, _, _ = sxe.initialize(model=model, config=ds)
    opt = eng.optimizer
    frozen_total = sum(p.ds_numel for n, p in model.named_parameters() if n in frozen_names)
    frozen_shard = sum((u.qshard[0].numel() if u.frozen_q else u.shard.numel()) for u in opt.frozen_units)
    frozen_bytes = sum((u.qshard[0].numel() * u.qshard[0].element_size() + u.qshard[1].numel() * 4)
                       if u.frozen_q else u.shard.numel() * u.shard.element_size() for u in opt.frozen_units)
    n_quant = sum(1 for u in opt.frozen_units if u.frozen_q)
    released = all(p.data.numel() == 0 for n, p in model.named_parameters() if n in frozen_names)
    before = full_params(eng)
    g = torch.Generator().manual_seed(11)
    losses = []
    for _ in range(steps):
        b = torch.randint(0, cfg.vocab_size, (world, 16), generator=g)[rank:rank + 1]
        loss = eng(b, labels=b)
        eng.backward(loss)
        eng.step()
        losses.append(float(loss.detach()))
    after = full_params(eng)
    eng.save_16bit_model(tmpdir, "frozen16.bin")
    saved = torch.load(os.path.join(tmpdir, "frozen16.bin"), weights_only=True) if rank == 0 else None
    frags = eng._frozen_param_fragments()
    return {"frozen_names": frozen_names, "frozen_total": frozen_total, "frozen_shard": frozen_shard,
            "frozen_bytes": frozen_bytes, "n_quant": n_quant, "n_frozen_units": len(opt.frozen_units),
            "released": released, "before": before, "after": after, "losses": losses,
            "saved_keys": sorted(saved) if saved is not None else None,
            "saved_frozen": {k: saved[k].float() for k in frozen_names} if saved is not None else None,
            "frag_keys": sorted(frags)}


def frozen_reference(before, frozen_names, steps, world, lr=1e-2):
    """Single-process reference of case_zero3_frozen from its initial weights, on the global batch."""
    from shuffle_exchange_amd.models import LlamaForCausalLM, llama_config
    cfg = llama_config("llama-tiny")
    model = LlamaForCausalLM(cfg).float()
    model.load_state_dict({k: v.float() for k, v in before.items()}, strict=False)
    for n, p in model.named_parameters():
        p.requires_grad_(n not in frozen_names)
    opt = torch.optim.AdamW([p for p in model.parameters() if p.requires_grad], lr=lr, weight_decay=0.0)
    g = torch.Generator().manual_seed(11)
    losses = []
    for _ in range(steps):
        b = torch.randint(0, cfg.vocab_size, (world, 16), generator=g)
        loss = model(b, labels=b)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return {n: q.detach().float().clone() for n, q in model.named_parameters()}, losses
