"""Distributed Lion optimizer (majority-vote sign aggregation), MI355X-native.

API-compatible with the reference ``Lion`` (/root/reference/distributed_lion.py:140-200):

    Lion(params, lr=1e-4, betas=(0.9, 0.99), weight_decay=0.0, max_grad_norm=None)

with the same ``state_dict`` schema (``state[p] == {'exp_avg': Tensor}`` in the
parameter dtype; group keys ``lr``, ``betas``, ``weight_decay``) and the same
update semantics, but a different execution model:

* one fused gfx950 kernel per *bucket* instead of ~20+6W ATen ops per tensor;
* the sign votes travel as true 1-bit planes in a few large collectives
  (``exchange=`` ``"allgather"`` | ``"a2a"`` | ``"ref_int64"``) instead of one
  int64 ``all_gather`` per tensor;
* the world size is resolved at every step (no stale dispatch) and
  defects D2-D5 of the reference are fixed.

Keyword-only extensions (all optional):
  vote         "majority" (reference) | "average" (paper's server averaging;
               with exchange="a2a" it travels as count bit planes at
               5 <= W <= 15 and over the all-gather otherwise)
  tie_break    "negative" (reference parity) | "zero" | "positive"
  param_rounding  "nearest" (reference parity) | "stochastic": how the update
               kernels store bf16 parameters.  Nearest drops an update below
               half a bf16 ulp (at lr 1e-4 every weight with |p| >= 2^-5 is
               frozen and the weight decay never acts); stochastic rounds
               fma(-lr, delta, p * (1 - lr*wd)) once, to one of its two bf16
               neighbours with probability proportional to the remainder, so
               the fp32 update survives in expectation.  The random bits are
               a hash of (seed, step count, global coordinate) without a rank
               term: replicas round identically.  The step count restarts on
               resume (like the stochastic encode's stream).  fp32 parameters
               are unaffected; fp16 parameters raise ValueError.
  exchange     vote exchange strategy, see parallel/exchange.py
  bucket_mb    packed-bit bucket size (MB) -- one collective per bucket.  None
               (default): at W > 1 the sign planes are cut into >= 4 buckets
               (each >= 1 MB, <= 32 MB) so bucket i's exchange overlaps bucket
               i+1's encode (and its shard vote / apply the neighbours'
               collectives); at W = 1 one 32 MB bucket size
  group        torch.distributed process group (default: WORLD)
  backend      "auto" | "hip" | "torch"
  seed         base seed of the stochastic-binarization RNG
  telemetry    collect vote-agreement counts (see :meth:`stats`)
  elastic_timeout  seconds; enables real worker-dropout handling: a heartbeat
               before each step's vote detects dead ranks and the survivors
               continue in a shrunken group (parallel/elastic.py)
"""
from __future__ import annotations

import hashlib
from typing import Callable, Dict, Optional, Sequence, Tuple

import torch
import torch.distributed as dist
from torch.optim.optimizer import Optimizer

from ..ops import reference as ref
from ..ops.linear import bump_weight_generation
from ..parallel.exchange import WireCounter, canonical_strategy, make_exchange, wire_bytes_per_step
from ..parallel.elastic import inject as inject_fault
from ..utils.timing import phase_of
from .executors import HParams, make_executor
from .plan import FlatPlan

# reference-compatible functional API re-exported from the oracle
update_fn = ref.update_fn
update_fn_distributed = ref.update_fn_distributed
update_fn_distributed_stoc = ref.update_fn_distributed_stoc
majority_vote = ref.majority_vote
flatten_and_pad = ref.flatten_and_pad
restore_flattened_tensor = ref.restore_flattened_tensor
exists = ref.exists


class Lion(Optimizer):
    def __init__(
        self,
        params,
        lr: float = 1e-4,
        betas: Tuple[float, float] = (0.9, 0.99),
        weight_decay: float = 0.0,
        max_grad_norm: Optional[float] = None,
        *,
        vote: str = "majority",
        tie_break: str = "negative",
        param_rounding: str = "nearest",
        exchange: str = "a2a",
        bucket_mb: Optional[float] = None,
        group=None,
        backend: str = "auto",
        seed: int = 0,
        telemetry: bool = False,
        verify_consistency: bool = True,
        elastic_timeout: Optional[float] = None,
    ):
        if not lr > 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not all(0.0 <= b <= 1.0 for b in betas):
            raise ValueError(f"Invalid betas: {betas}")
        if max_grad_norm is not None and not max_grad_norm > 0:
            raise ValueError(f"Invalid max_grad_norm: {max_grad_norm}")
        if vote not in ref.VOTE_CODES:
            raise ValueError(f"vote must be one of {tuple(ref.VOTE_CODES)}")
        if tie_break not in ref.TIE_CODES:
            raise ValueError(f"tie_break must be one of {tuple(ref.TIE_CODES)}")
        if param_rounding not in ref.ROUNDING_CODES:
            raise ValueError(f"param_rounding must be one of {tuple(ref.ROUNDING_CODES)}")
        defaults = dict(lr=lr, betas=betas, weight_decay=weight_decay)
        super().__init__(params, defaults)
        # stored (reference D2: it never was) but, like the reference, not part of state_dict
        self.max_grad_norm = max_grad_norm
        self.vote = vote
        self.tie_break = tie_break
        self.param_rounding = param_rounding
        self.exchange_name = canonical_strategy(exchange)
        self.bucket_bytes = None if bucket_mb is None else int(bucket_mb * (1 << 20))
        self.process_group = group
        self.backend = backend
        self.seed = int(seed)
        self.telemetry = telemetry
        self.verify_consistency = verify_consistency
        self._n_steps = 0
        self._plan: Optional[FlatPlan] = None
        self._executor = None
        self._exchange = None
        self._alive_host: Optional[Tuple[bool, ...]] = None
        self._alive_dev: Optional[torch.Tensor] = None
        self._dropped: set = set()
        self._dropout_schedule: Dict[int, Sequence[int]] = {}
        self._agree: Optional[torch.Tensor] = None
        self._agree_coords = 0  # coordinates covered by the agreement counter since the last stats()
        self._tie_coords = 0
        self.last_world = 1
        self.elastic_timeout = elastic_timeout
        self._elastic = None
        # optional utils.metrics.PhaseTimer: encode / exchange / apply (local_update at W=1)
        self.phase_timer = None
        # run the vote path (encode -> collectives -> apply) even on a 1-rank
        # group: exercises the RCCL calls on a single GPU (tests/test_nccl_gpu.py)
        self._force_vote = False
        # route a2a + average over the count planes at any W <= 15 (by default
        # only where they move fewer bytes than the all-gather, W >= 5)
        self._force_counts = False
        self._wire_carry = WireCounter()  # counts of exchanges replaced after a regroup

    # ------------------------------------------------------------ topology
    def _world(self):
        """(world, rank) resolved now -- never cached."""
        if not (dist.is_available() and dist.is_initialized()):
            return 1, 0
        g = self.process_group
        return dist.get_world_size(g), dist.get_rank(g)

    # ------------------------------------------------------ worker dropout
    def drop_workers(self, ranks: Sequence[int]) -> None:
        """Exclude ``ranks`` from every subsequent vote (simulated dropout /
        abstention).  Must be called identically on every rank; the dropped
        ranks keep running the collective so nothing hangs, but their planes
        are ignored and the majority is taken over the live voters only."""
        self._dropped |= {int(r) for r in ranks}

    def restore_workers(self, ranks: Optional[Sequence[int]] = None) -> None:
        if ranks is None:
            self._dropped.clear()
        else:
            self._dropped -= {int(r) for r in ranks}

    def set_dropout_schedule(self, schedule: Dict[int, Sequence[int]]) -> None:
        """{step: [ranks to drop from that optimizer step on]} (fault injection)."""
        self._dropout_schedule = {int(k): list(v) for k, v in schedule.items()}

    def _alive(self, world: int, device) -> torch.Tensor:
        if self._n_steps in self._dropout_schedule:
            self.drop_workers(self._dropout_schedule[self._n_steps])
        host = tuple(r not in self._dropped for r in range(world))
        if not any(host):
            # with no live voter the exchanges would disagree (allgather: delta 0,
            # a2a without a negative plane: delta -1), so this is refused outright
            raise ValueError(f"every worker of the {world}-rank vote is dropped ({sorted(self._dropped)}); "
                             "at least one rank must keep voting")
        if self._alive_dev is None or host != self._alive_host or self._alive_dev.device != device:
            t = torch.tensor([1 if a else 0 for a in host], dtype=torch.uint8)
            self._alive_dev = t.to(device)
            self._alive_host = host
        return self._alive_dev

    def _elastic_setup(self) -> None:
        """Real dropout (``elastic_timeout``): every vote runs as a guarded,
        store-committed collective on the default group (parallel/elastic.py);
        after a regroup the plan is rebuilt for the survivors' world."""
        if self.elastic_timeout is None or not (dist.is_available() and dist.is_initialized()):
            return
        from ..parallel.elastic import ElasticGroup

        if self.process_group is not None:
            raise ValueError("elastic_timeout works on the default process group (group=None)")
        if self.exchange_name == "ref_int64":
            raise ValueError("the ref_int64 wire issues blocking per-tensor collectives; it cannot be "
                             "elastic -- use exchange='a2a' or 'allgather'")
        el = ElasticGroup.get(self.elastic_timeout)
        if self._elastic is not el:
            self._elastic = el
            el.on_regroup(self._on_regroup)

    def _on_regroup(self, el) -> None:
        if self._exchange is not None:  # keep the wire counts of the abandoned exchange
            w = self._exchange.wire
            self._wire_carry.add(w.sent, w.recv, w.calls)
        self._plan = None  # re-planned for the new world at the next step
        self._exchange = None
        self._dropped.clear()  # simulated-dropout ranks were numbered in the old group
        self._alive_dev = None

    # --------------------------------------------------------------- plan
    def _get_plan(self, entries, world: int, rank: int):
        key = (FlatPlan.make_key(entries), world, self.exchange_name)
        if self._plan is not None and getattr(self._plan, "_full_key", None) == key:
            return self._plan
        backend = None
        if world > 1 and dist.is_initialized():
            try:
                backend = dist.get_backend(self.process_group)
            except (RuntimeError, ValueError):  # a simulated group has no c10d backend name
                backend = None
        if self.param_rounding == "stochastic" and any(p.dtype == torch.float16 for p, _ in entries):
            raise ValueError("param_rounding='stochastic' supports bfloat16 parameters (float32 ones are stored "
                             "exactly either way), not float16")
        plan = FlatPlan(entries, world=world, bucket_bytes=self._bucket_bytes(entries, world, backend))
        plan._full_key = key
        self._plan = plan
        self._executor = make_executor(plan, self.backend)
        if world > 1 or self._force_vote:
            if self.verify_consistency:
                self._check_consistency(plan)
            self._exchange = make_exchange(self.exchange_name, plan, self.process_group, rank, world,
                                           self._executor, ref.TIE_CODES[self.tie_break],
                                           ref.VOTE_CODES[self.vote], counts=self._counts_arg())
        else:
            self._exchange = None
        return plan

    def _counts_arg(self) -> Optional[bool]:
        return True if self._force_counts else None

    # automatic bucket size (bucket_mb=None): 32 MB planes at most (Llama-3-8B:
    # 1 GB of sign bits -> 32 buckets), at least MIN_BUCKETS per step at W > 1
    # (GPT-2: 15.6 MB -> one 32 MB bucket would serialise encode -> a2a ->
    # shard vote -> all-gather -> apply), and no collective payload under 1 MB.
    # gloo runs every collective on the host (device -> host copy, TCP, back):
    # each extra bucket costs tens of ms there, so gloo keeps the largest
    # buckets (8 gloo ranks on one GPU, GPT-2: exposed exchange 51 ms with one
    # bucket, 277-413 ms with 4, 1016 ms with 13 -- profiles/r4/bucket_sweep_w8_gloo.txt)
    MAX_BUCKET_BYTES = 32 << 20
    MIN_BUCKET_BYTES = 1 << 20
    MIN_BUCKETS = 4

    def _bucket_bytes(self, entries, world: int, backend: Optional[str] = None) -> int:
        if self.bucket_bytes is not None:
            return self.bucket_bytes
        if (world <= 1 and not self._force_vote) or backend == "gloo":
            return self.MAX_BUCKET_BYTES
        from .plan import ALIGN_ELEMS

        total = sum((p.numel() + ALIGN_ELEMS - 1) // ALIGN_ELEMS * ALIGN_ELEMS // 8 for p, _ in entries)
        per = -(-total // self.MIN_BUCKETS)
        return int(min(self.MAX_BUCKET_BYTES, max(self.MIN_BUCKET_BYTES, per)))

    def _check_consistency(self, plan: FlatPlan) -> None:
        """All ranks must vote on the same tensors in the same order, or the
        collectives silently mismatch.  One tiny all-reduce per
        new plan compares a digest of the layout."""
        h = hashlib.sha256()
        for s in plan.segments:
            h.update(f"{s.numel}:{s.param.dtype}:{s.bit_off};".encode())
        for b in plan.buckets:
            h.update(f"B{b.nbytes}:{b.group};".encode())
        v = int.from_bytes(h.digest()[:7], "little")
        dev = plan.device if dist.get_backend(self.process_group) == "nccl" else torch.device("cpu")
        t = torch.tensor([v, -v], dtype=torch.int64, device=dev)
        if self._elastic is not None:
            self._elastic.all_reduce(t, op=dist.ReduceOp.MAX)
        else:
            dist.all_reduce(t, op=dist.ReduceOp.MAX, group=self.process_group)
        if int(t[0]) != v or int(t[1]) != -v:
            raise RuntimeError(
                "dlion Lion: parameter/gradient layout differs across ranks (different params have grads?); "
                "the vote collectives would mismatch")

    # --------------------------------------------------------------- step
    def _collect(self):
        entries, grads, moms = [], [], []
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError("Lion does not support sparse gradients")
                state = self.state[p]
                if len(state) == 0:
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                entries.append((p, gi))
                grads.append(g)
                moms.append(state["exp_avg"])
        return entries, grads, moms

    @torch.no_grad()
    def clip_grad_norm_(self, max_norm: float) -> torch.Tensor:
        """Fused ``torch.nn.utils.clip_grad_norm_(params, max_norm)`` (L2) over
        this optimizer's gradients.  On the HIP path the norm is one read of
        every gradient through the update kernels' pointer table, the clip
        coefficient stays on the device (no host sync) and the NEXT ``step()``
        applies ``g * coef`` (rounded to the gradient dtype, exactly what the
        in-place ``_foreach_mul_`` would have stored) inside its kernels --
        instead of a separate read+write pass over all gradients (measured on
        Llama-3-8B: 19.5 ms of foreach norm+mul per step).  The coefficient is
        computed in fp32 (torch computes bf16 gradients' norms in bf16).  The
        gradients themselves are left unscaled; call ``step()`` next.
        Returns the total norm (0-dim device tensor)."""
        entries, grads, moms = self._collect()
        if not entries:
            return torch.zeros(())
        world, rank = self._world()
        plan = self._get_plan(entries, world, rank)
        ex = self._executor
        if ex.name != "hip":
            self._pending_gscale = None
            return torch.nn.utils.clip_grad_norm_([p for p, _ in entries], max_norm)
        meta = plan.meta(grads, moms)
        n = plan.total_chunks
        if getattr(self, "_clip_part", None) is None or self._clip_part.numel() < n or \
                self._clip_part.device != plan.device:
            self._clip_part = torch.empty(n, dtype=torch.float32, device=plan.device)
            self._clip_out = torch.empty(2, dtype=torch.float32, device=plan.device)
        for b in plan.buckets:
            ex.grad_sumsq(meta, b, self._clip_part)
        ex.clip_coef(self._clip_part, n, float(max_norm), self._clip_out)
        self._pending_gscale = self._clip_out
        return self._clip_out[0]

    @torch.no_grad()
    def step(self, closure: Optional[Callable] = None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()

        entries, grads, moms = self._collect()
        if not entries:
            return loss

        inject_fault("before_step", self._n_steps)
        self._elastic_setup()
        world, rank = self._world()
        self.last_world = world
        plan = self._get_plan(entries, world, rank)
        ex = self._executor
        meta = plan.meta(grads, moms) if ex.name == "hip" else None
        hps = [HParams(lr=g["lr"], wd=g["weight_decay"], beta1=g["betas"][0], beta2=g["betas"][1])
               for g in self.param_groups]

        gscale, self._pending_gscale = getattr(self, "_pending_gscale", None), None
        if world == 1 and not self._force_vote:
            with phase_of(self.phase_timer, "local_update"):
                for b in plan.buckets:
                    ex.local(meta, b, hps[b.group], grads=grads, moms=moms, gscale=gscale, **self._rounding_kw())
        else:
            self._distributed_step(plan, ex, meta, hps, grads, moms, world, rank, gscale)
        # the kernels wrote the weights through raw pointers (no autograd
        # version bump): invalidate derived per-step weight copies
        bump_weight_generation()
        self._n_steps += 1
        return loss

    def _distributed_step(self, plan, ex, meta, hps, grads, moms, world, rank, gscale=None):
        if self._elastic is not None:
            return self._elastic_step(plan, ex, meta, hps, grads, moms, world, rank, gscale)
        xch, t = self._exchange, self.phase_timer
        alive = self._alive(world, plan.device)
        self._telemetry_setup(plan, xch)
        # encode bucket i, then its collective overlaps the encode of i+1
        states, _ = self._encode_launch(plan, ex, meta, hps, grads, moms, rank, gscale, alive)
        with phase_of(t, "exchange"):
            states = [xch.advance(b, s, alive) for b, s in zip(plan.buckets, states)]
        for b, s in zip(plan.buckets, states):
            with phase_of(t, "exchange"):
                a = xch.finish(b, s, alive)
            with phase_of(t, "apply"):
                ex.apply(meta, b, a.planes, a.stride, alive, a.mode, ref.TIE_CODES[self.tie_break], a.neg,
                         hps[b.group], own=xch.send_view(b) if self.telemetry else None,
                         agree=self._agree if self.telemetry else None, **self._rounding_kw())

    def _rounding_kw(self) -> dict:
        """The parameter-store rounding of this step: keyed on (seed, step
        count) only, so every rank -- and a re-vote of the same step -- rounds
        the same way."""
        return dict(rounding=ref.ROUNDING_CODES[self.param_rounding], seed=self.seed, step=self._n_steps)

    def _telemetry_setup(self, plan, xch) -> None:
        """telemetry: [agreements, ties] counters on the device, and the number
        of coordinates they cover (this rank votes on all of them, or on its
        1/W shard under a2a, where K4 counts the ties)."""
        if not self.telemetry:
            return
        if self._agree is None or self._agree.device != plan.device:
            self._agree = torch.zeros(2, dtype=torch.int64, device=plan.device)
        if xch is not None and hasattr(xch, "need_neg"):  # a2a
            xch.ties = self._agree[1:2]
            self._tie_coords += sum(b.nbytes * 8 // xch.world for b in plan.buckets)
        else:
            self._tie_coords += sum(s.numel for s in plan.segments)
        self._agree_coords += sum(s.numel for s in plan.segments)

    def _encode_launch(self, plan, ex, meta, hps, grads, moms, rank, gscale, alive, guarded=False):
        """Encode bucket i, then launch its collective (it overlaps the encode
        of bucket i+1).  ``guarded`` (elastic mode): a launch that raises (a
        broken group reports a dead peer at issue time) stops further launches
        but NOT the encodes -- every bucket's momentum must advance exactly
        once and every sign plane must be this step's, because the survivors'
        re-vote all-gathers the whole send buffer as it stands.  Returns
        ``(states, launch_error)``."""
        xch, stochastic, t = self._exchange, self.max_grad_norm is not None, self.phase_timer
        seed = (self.seed * 0x9E3779B1 + rank * 0x632BE59BD9B4E019 + 1) & 0x7FFFFFFFFFFFFFFF
        states, err = [], None
        for b in plan.buckets:
            hp = hps[b.group]
            rr = (1.0 + 1.0 / hp.beta1) * self.max_grad_norm if stochastic else 0.0
            with phase_of(t, "encode"):
                ex.encode(meta, b, xch.send_view(b), hp, update_m=True, stochastic=stochastic, rr=rr, seed=seed,
                          step=self._n_steps, grads=grads, moms=moms, gscale=gscale)
                if err is not None:
                    states.append(None)
                    continue
                try:
                    if b.index == 1:
                        inject_fault("raise_in_launch", self._n_steps)
                    states.append(xch.launch(b, alive))
                except Exception as e:  # noqa: BLE001 - re-raised unless guarded
                    if not guarded:
                        raise
                    err = e
                    states.append(None)
                    continue
            if b.index == 0:
                inject_fault("after_launch", self._n_steps)
        return states, err

    def _elastic_step(self, plan, ex, meta, hps, grads, moms, world, rank, gscale=None):
        """The vote as guarded collectives: the host polls each phase to
        completion (bounded by ``elastic_timeout``) before anything on the
        compute stream depends on it, and applies the step only after the
        store-arbitrated commit.  On a failure the survivors regroup and vote
        again from the intact encoded planes (the momentum was already
        advanced by the encode, exactly once) with a 1-bit all-gather over
        the new group, on the old plan's layout."""
        from ..parallel.elastic import flatten_works

        el, xch, t = self._elastic, self._exchange, self.phase_timer
        alive = self._alive(world, plan.device)
        self._telemetry_setup(plan, xch)
        tie = ref.TIE_CODES[self.tie_break]
        ok = True
        try:
            states, err = self._encode_launch(plan, ex, meta, hps, grads, moms, rank, gscale, alive, guarded=True)
            if err is not None:
                raise err
            with phase_of(t, "exchange"):
                ok = el.wait_works(flatten_works(states))
                if ok:
                    states = [xch.advance(b, s, alive) for b, s in zip(plan.buckets, states)]
                    inject_fault("in_allgather", self._n_steps)
                    ok = el.wait_works(flatten_works(states))
        except Exception as e:  # noqa: BLE001 - gloo reports a dead peer at issue time
            import logging

            logging.getLogger(__name__).warning("dlion: vote collective failed: %s", str(e)[:200])
            ok = False
        with phase_of(t, "exchange"):
            committed = el.commit(ok)
        if committed:
            for b, s in zip(plan.buckets, states):
                a = xch.finish(b, s, alive)
                with phase_of(t, "apply"):
                    ex.apply(meta, b, a.planes, a.stride, alive, a.mode, tie, a.neg, hps[b.group],
                             own=xch.send_view(b) if self.telemetry else None,
                             agree=self._agree if self.telemetry else None, **self._rounding_kw())
            inject_fault("after_vote", self._n_steps)
            return
        # ---- somebody failed: regroup, then vote again among the survivors
        from ..parallel.exchange import AllGatherExchange

        send = xch.send
        while True:
            el.regroup({"step": self._n_steps, "where": "vote"})
            w2, r2 = el.world, el.rank
            if w2 == 1:  # the last one standing votes alone: its own signs
                rex, alive2 = None, torch.ones(1, dtype=torch.uint8, device=plan.device)
                break
            alive2 = torch.ones(w2, dtype=torch.uint8, device=plan.device)
            rex = AllGatherExchange(plan, None, r2, w2, ex, tie, ref.VOTE_CODES[self.vote], send=send)
            try:
                works = [rex.launch(b, alive2) for b in plan.buckets]
                ok = el.wait_works(works)
            except Exception:  # noqa: BLE001
                ok = False
            if el.commit(ok):
                break
        for b in plan.buckets:
            if rex is None:
                planes, stride, mode = send[b.byte_off:b.byte_off + b.nbytes], b.nbytes, ref.VOTE_CODES[self.vote]
            else:
                a = rex.finish(b, None, alive2)
                planes, stride, mode = a.planes, a.stride, a.mode
            ex.apply(meta, b, planes, stride, alive2, mode, tie, None, hps[b.group], **self._rounding_kw())
        if rex is not None:
            self._wire_carry.add(rex.wire.sent, rex.wire.recv, rex.wire.calls)

    # ---------------------------------------------------------- telemetry
    def stats(self, reset: bool = True) -> dict:
        """Wire counters and (telemetry=True) vote agreement since last reset.
        Reading the agreement count synchronises with the device."""
        out = {"world": self.last_world, "exchange": self.exchange_name, "steps": self._n_steps,
               "param_rounding": self.param_rounding}
        if self._exchange is not None or self._wire_carry.calls:
            tot = WireCounter()
            for w in (self._wire_carry, getattr(self._exchange, "wire", None)):
                if w is not None:
                    tot.add(w.sent, w.recv, w.calls)
                    if reset:
                        w.reset()
            out.update(tot.snapshot())
        if self._executor is not None:
            out["executor"] = type(self._executor).__name__  # HipExecutor: the gfx950 kernels ran
        if self._plan is not None:
            out["numel"] = sum(s.numel for s in self._plan.segments)
            out["n_buckets"] = len(self._plan.buckets)
            out["wire_bytes_analytic"] = wire_bytes_per_step(out["numel"], self.last_world, self.exchange_name,
                                                             vote=self.vote, counts=self._counts_arg())
        if self._exchange is not None:
            out["exchange_impl"] = type(self._exchange).__name__ + (
                "+counts" if getattr(self._exchange, "use_counts", False) else "")
        if self._elastic is not None:
            out.update(self._elastic.stats())
        if self._agree is not None:
            agree, ties = (int(x) for x in self._agree.tolist())  # one device sync (telemetry only)
            out["vote_agree"] = agree
            out["vote_ties"] = ties
            out["vote_agree_rate"] = agree / max(1, self._agree_coords)
            out["vote_tie_rate"] = ties / max(1, self._tie_coords)
            if reset:
                self._agree.zero_()
                self._agree_coords = self._tie_coords = 0
        return out

    @property
    def plan(self) -> Optional[FlatPlan]:
        return self._plan
