"""FusedSAC, FusedTD3, FusedDDPG: the reference's three learners (pytorch_sac_temp/sac.py, pytorch_td3_temp/td3.py,
pytorch_ddpg_temp/ddpg.py) with every step of update_parameters as HIP launches of libuavx_actor.so:

    sample   FusedReplaySampler on a DeviceReplay                          (§16)
             (NStepReplaySampler with n_step > 1 or recency > 0: n-step returns, recency-weighted draws, §22;
              PrioritizedReplaySampler with prioritized=alpha: proportional draws, |q - y| fed back as priorities, §23;
              with per_beta > 0 its importance-sampling weights multiply the critic loss row by row, §24;
              with per_n_step > 1 PrioritizedNStepSampler: n-step returns walked from the drawn transitions, §25)
    target   FusedTarget: next action, target critic, y                    (§13)
    critic   FusedCriticLoss into .grad, FusedAdam step                    (§14, §15)
    actor    FusedPolicyGrad into .grad, FusedAdam step, soft updates      (§17, §18, §15)
    tail     SAC's alpha step and the loss record (include/uavx_learner.h) (§19)

    agent = FusedSAC(memory=mem)                       # constructor keywords and attribute names of the reference's SAC
    agent.update_parameters(mem, 256)                  # one update, eager; returns nothing, syncs nothing
    agent.capture(256); agent.run(1000)                # the same update as a captured graph, replayed
    agent.losses(last=10)                              # the ONE host read: [n, 8] rows of the loss ring, in update order
    a = agent.select_action(mem.state)                 # FusedActor.act on the live actor
    sd = agent.state_dict(); agent.load_state_dict(sd) # the whole learner, for checkpoint.save_run / load_run (§27)

A row of the loss ring holds critic_loss_1, critic_loss_2 (0 for DDPG), actor_loss (0 in an update without an actor
step), alpha_loss, alpha, actor_updated, 0, 0: what the reference's update_parameters returns through .item().

One deliberate difference from the reference: sac.py:29 reads its target_entropy from an uninitialised tensor
(torch.Tensor(n_actions) with an int); FusedSAC takes target_entropy=None -> -float(n_actions), the value the comment at
sac.py:28 intends.  Everything else follows the reference, its quirks included: SAC's update 0 uses alpha = `alpah` (2)
and later updates exp(log_alpha); TD3 steps the actor and both targets only when updates % policy_freq == 0.
There is NO fallback: anything the kernels do not implement raises before a launch."""
import ctypes
import math
import operator
import os

import torch

from . import _actor_lib, policy
from ._fused_common import capture_guard, check_f32, column, rows2, stream
from .fused_actor import FusedActor
from .fused_critic import FusedCritic, FusedCriticLoss, FusedTarget
from .fused_optim import FusedAdam, check_max_grad_norm, soft_update
from .fused_policy_grad import FusedPolicyGrad
from .fused_replay import FusedReplaySampler
from .fused_replay_nstep import N_STEP_MAX, NStepReplaySampler, check_n_step
from .prioritized_nstep import PrioritizedNStepSampler
from .prioritized_replay import PrioritizedReplaySampler, check_prioritized
from .replay import DeviceReplay

LOG_COLUMNS = _actor_lib.LEARNER_LOG_COLUMNS
COLUMNS = ("critic_loss_1", "critic_loss_2", "actor_loss", "alpha_loss", "alpha", "actor_updated")
_CLIP_RECORD = 6         # float32 elements of a FusedAdam clip record: norm, coef, the int64 count, the bound, padding


def _cpu(x):
    """A state dict (module's or optimiser's) with every tensor detached and on the CPU."""
    if torch.is_tensor(x):
        return x.detach().cpu()
    if isinstance(x, dict):
        return {k: _cpu(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(_cpu(v) for v in x)
    return x


def ddpg_init(net, init_w):
    """pytorch_ddpg_temp/model.py's init_weights on a DDPGActor / DDPGCritic: `input` and `fc1` weights from
    U(+-1/sqrt(size[0])), size[0] being the layer's OUT features (fanin_init's quirk, model.py:62-65), `fc2`'s from
    U(+-init_w) (5e-4 for the actor, 5e-5 for the critic); the biases keep nn.Linear's default, as there."""
    with torch.no_grad():
        for lin in (net.input, net.fc1):
            b = 1.0 / math.sqrt(lin.weight.shape[0])
            lin.weight.uniform_(-b, b)
        net.fc2.weight.uniform_(-init_w, init_w)
    return net


def _copy_params(target, source):
    with torch.no_grad():
        for t, s in zip(target.parameters(), source.parameters()):
            t.copy_(s)


def _amend(path, entries):
    """Adds / replaces entries of a checkpoint file one of policy.py's savers wrote (tensors stored on the CPU)."""
    ck = torch.load(path, map_location="cpu", weights_only=True)
    ck.update(entries)
    torch.save(ck, path)


class _FusedLearner:
    """What the three learners share: the loss ring, the tail launch, sampling, capture / run and the batch checks."""
    kind = None
    _noises = 0          # [B, 2] standard-normal tensors one update consumes

    def _setup(self, device, generator, log_capacity, memory, n_step=1, recency=0.0, prioritized=None, per_eps=1e-6,
               per_beta=0.0, per_n_step=1, max_grad_norm=None):
        self.n_step, self.recency = check_n_step(n_step, recency, type(self).__name__)
        self.max_grad_norm = self._check_max_grad_norm(max_grad_norm)
        self.prioritized = self.per_eps = None
        if prioritized is not None:
            self.prioritized, self.per_eps = check_prioritized(prioritized, per_eps, type(self).__name__)
            if self.n_step != 1 or self.recency != 0.0:
                raise ValueError(f"uavx: {type(self).__name__} draws prioritized batches one step at a time: prioritized="
                                 f"{prioritized} goes with n_step=1 and recency=0, not n_step={self.n_step}, "
                                 f"recency={self.recency}")
        self.per_beta = self._check_per_beta(per_beta)
        if self.per_beta > 0.0 and self.prioritized is None:
            raise ValueError(f"uavx: {type(self).__name__} weights the critic loss of prioritized batches: per_beta="
                             f"{per_beta} needs prioritized=alpha")
        # per_beta > 0 at construction picks the weighted update (§24) for the learner's life; set_per_beta moves beta in it
        self._per_weighted = self.per_beta > 0.0
        self.per_n_step = self._check_per_n_step(per_n_step)
        if self.per_n_step > 1 and self.prioritized is None:
            raise ValueError(f"uavx: {type(self).__name__} walks n steps from the keys of prioritized batches: per_n_step="
                             f"{per_n_step} needs prioritized=alpha (n_step is the uniform sampler's)")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"uavx: the learners need a GPU (cuda:N), got {self.device}: there is no CPU path")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if generator is not None and generator.device != self.device:
            raise ValueError(f"uavx: generator is on {generator.device}, the learner on {self.device}")
        log_capacity = int(log_capacity)
        if log_capacity < 1:
            raise ValueError(f"uavx: log_capacity must be >= 1, got {log_capacity}")
        self.generator, self.log_capacity = generator, log_capacity
        self._lib = _actor_lib.load()
        # the loss ring and, behind it in the same allocation, the int64 count the tail launch advances and the two
        # optimisers' clip records (critic's, actor's; §26): one copy reads them all
        n = log_capacity * LOG_COLUMNS
        self._ring = torch.zeros(n + 2 + 2 * _CLIP_RECORD, dtype=torch.float32, device=self.device)
        self._log = self._ring[:n].view(log_capacity, LOG_COLUMNS)
        self._updates = self._ring[n:n + 2].view(torch.int64)
        self._clip_recs = tuple(self._ring[n + 2 + k * _CLIP_RECORD:n + 2 + (k + 1) * _CLIP_RECORD] for k in range(2))
        self.updates = 0                  # the host's count of updates enqueued: what `updates=None` stands for
        self._losses_in = (ctypes.c_void_p * 3)()
        self._sampler = self._batch = self._y = None
        self._qbuf = {}       # rows -> (q [towers, rows], dq/da [towers, rows, 2]) of the priority feedback
        self._graphs = None
        self.memory = None
        if memory is not None:
            self.attach(memory)

    # ---- pieces the subclasses name -----------------------------------------------------------------------------------
    def _pieces(self):
        """(FusedCriticLoss, FusedPolicyGrad): what reserve() sizes."""
        return self._closs, self._pgrad

    def _variants(self):
        """The `full` flags an update can run with: one graph is captured for each."""
        return (True,)

    def _full(self, updates):
        return True

    def _update(self, s, a, r, s2, mask, noise, full, key=None, weight=None):
        raise NotImplementedError

    # ---- priorities ---------------------------------------------------------------------------------------------------
    def _check_per_beta(self, beta):
        """The importance-sampling exponent as a float: finite, in [0, 1]."""
        try:
            b = float(beta)
        except (TypeError, ValueError):
            b = float("nan")                 # refused below
        if not 0.0 <= b <= 1.0:
            raise ValueError(f"uavx: {type(self).__name__} takes an importance-sampling exponent per_beta in [0, 1], got "
                             f"{beta}")
        return b

    def _check_per_n_step(self, n):
        """The steps a prioritized batch walks from each drawn transition, as an int in 1..8 (a bool is not a count)."""
        try:
            k = 0 if isinstance(n, bool) else operator.index(n)
        except TypeError:
            k = 0
        if not 1 <= k <= N_STEP_MAX:
            raise ValueError(f"uavx: {type(self).__name__} takes per_n_step as an integer in 1..{N_STEP_MAX}, got {n!r}")
        return k

    def set_per_beta(self, beta):
        """Moves the importance-sampling exponent of a learner built with per_beta > 0 (an annealed beta): the sampler
        keeps it in a device slot, so a captured update follows it.  A learner built with per_beta == 0 runs the
        unweighted update, which reads no weights, and refuses."""
        beta = self._check_per_beta(beta)
        if not self._per_weighted:
            raise ValueError(f"uavx: set_per_beta needs a {type(self).__name__} built with prioritized=alpha and "
                             f"per_beta > 0: this one runs the unweighted update")
        self.per_beta = beta
        if self._sampler is not None:
            self._sampler.set_beta(beta)
        return self

    # ---- gradient-norm clipping (§26) -----------------------------------------------------------------------------------
    def _check_max_grad_norm(self, x):
        """max_grad_norm as (the critic optimiser's bound, the actor optimiser's), each a float or None: a float stands for
        both, a pair (critic, actor) names them one by one."""
        what = f"{type(self).__name__}: max_grad_norm"
        if x is None:
            return (None, None)
        if isinstance(x, (tuple, list)):
            if len(x) != 2:
                raise ValueError(f"uavx: {what} is a float or a pair (critic, actor), got {len(x)} entries")
            return tuple(None if v is None else check_max_grad_norm(v, what) for v in x)
        return (check_max_grad_norm(x, what),) * 2

    def _adams(self):
        """(the critic's FusedAdam, the actor's)."""
        raise NotImplementedError

    def _clip_kw(self, k):
        """FusedAdam's clipping keywords for optimiser k (0 the critic's, 1 the actor's): its record lies behind the loss
        ring.  Nothing for an unclipped one, which then makes the calls it always made."""
        bound = self.max_grad_norm[k]
        return {} if bound is None else dict(max_grad_norm=bound, record=self._clip_recs[k])

    def set_max_grad_norm(self, max_grad_norm):
        """Moves the clip bounds of a learner built with max_grad_norm (a float for both optimisers, or a pair (critic,
        actor) in which None leaves that one as it is); the bounds live in device slots, so a captured update follows them.
        An optimiser built without clipping runs the unclipped step and refuses a bound."""
        new = self._check_max_grad_norm(max_grad_norm)
        for adam, bound, name in zip(self._adams(), new, ("critic", "actor")):
            if bound is not None and adam.max_grad_norm is None:
                raise ValueError(f"uavx: set_max_grad_norm needs a {type(self).__name__} whose {name} optimiser was built "
                                 f"with max_grad_norm: this one runs the unclipped step")
        for adam, bound in zip(self._adams(), new):
            if bound is not None:
                adam.set_max_grad_norm(bound)
        self.max_grad_norm = tuple(a.max_grad_norm for a in self._adams())
        return self

    def grad_norms(self):
        """{"critic": (grad_norm, clip_coef, clipped_steps), "actor": (...)} of the optimisers' last steps as 0-d device
        views (no host synchronisation; reading one does synchronise); None for an optimiser that does not clip."""
        return {name: None if a.max_grad_norm is None else (a.grad_norm, a.clip_coef, a.clipped_steps)
                for name, a in zip(("critic", "actor"), self._adams())}

    def _q_out(self, rows):
        """The feedback's (q, dq/da) buffers for `rows` rows: reserved ones, or new ones outside a capture.  The weighted
        update takes q from the critic gradient itself and has no dq/da (None)."""
        if rows not in self._qbuf:
            capture_guard("buffers", rows)
            towers = self._pgrad.critic.critic.towers
            self._qbuf[rows] = (torch.empty((towers, rows), dtype=torch.float32, device=self.device),
                                None if self._per_weighted else
                                torch.empty((towers, rows, 2), dtype=torch.float32, device=self.device))
        return self._qbuf[rows]

    def _check_key(self, key, rows):
        """What update_batch refuses about its keys, before the update computes or draws anything."""
        if not isinstance(self._sampler, PrioritizedReplaySampler):
            raise ValueError(f"uavx: keys need a {type(self).__name__} built with prioritized=alpha and a DeviceReplay")
        if (not torch.is_tensor(key) or key.dtype != torch.int64 or tuple(key.shape) != (rows,) or key.device != self.device
                or not key.is_contiguous()):
            raise ValueError(f"uavx: key must be a contiguous int64 tensor of shape [{rows}] on {self.device}")

    def _feedback(self, s, a, y, key):
        """Between the target and the critic's step: q(s, a) of the LIVE critic (FusedActionGrad.q_dqda, one launch) and
        max over its towers of |q - y| into the priorities of the sampled transitions.  key: None (nothing happens), or
        (the sampler's keys, whether the kernels read the ring's fill from the device count)."""
        if key is None:
            return
        key, device_count = key
        out = self._q_out(s.shape[0])
        self._pgrad.critic.q_dqda(s, a, out=out)
        self._sampler.update_priorities(key, out[0], y, device_count=device_count)

    def _critic_grad(self, s, a, y, key, weight):
        """The priority feedback and the critic gradient of one update -> the critic loss.  Without a weight, in a learner
        built with per_beta == 0: _feedback, then the unweighted gradient.  Otherwise (§24) the weighted gradient, whose row
        pass hands back q(s, a) of the live critic for update_priorities: no q_dqda launch."""
        if weight is None and not self._per_weighted:
            self._feedback(s, a, y, key)
            return self._closs.backward(s, a, y)
        q = None if key is None else self._q_out(s.shape[0])[0]
        loss = self._closs.backward(s, a, y, weight=weight, q_out=q)
        if key is not None:
            self._sampler.update_priorities(key[0], q, y, device_count=key[1])
        return loss

    # ---- the tail -----------------------------------------------------------------------------------------------------
    def _tail(self, critic_loss, actor_loss, sac=None):
        """One launch: the loss row, the update count and (sac = (log_pi_mean, hyper) with automatic entropy tuning)
        the alpha step.  critic_loss: what FusedCriticLoss.backward returned (0-d device views, two for a twin critic);
        actor_loss: FusedPolicyGrad's, or None in an update without an actor step."""
        li = self._losses_in
        twin = isinstance(critic_loss, tuple)
        li[0] = (critic_loss[0] if twin else critic_loss).data_ptr()
        li[1] = critic_loss[1].data_ptr() if twin else None
        li[2] = None if actor_loss is None else actor_loss.data_ptr()
        alpha = getattr(self, "_alpha", None)
        if sac is None:
            args = (None, 0.0, None, None, None, None, 0.0, 0.0, 0.0, 0.0)
        else:
            lpm, (lr, b1, b2, eps) = sac
            st = self.alpha_optim.state[self.log_alpha]
            args = (lpm.data_ptr(), self.target_entropy, self.log_alpha.data_ptr(), st["exp_avg"].data_ptr(),
                    st["exp_avg_sq"].data_ptr(), self._alpha_adam.step_pointer(), lr, b1, b2, eps)
        with torch.cuda.device(self.device):
            rc = self._lib.uavx_learner_tail(self.kind, li, *args, None if alpha is None else alpha.data_ptr(),
                                             self._log.data_ptr(), self.log_capacity, self._updates.data_ptr(),
                                             int(actor_loss is not None), stream(self.device))
        _actor_lib.check(rc, "uavx_learner_tail")

    # ---- batches ------------------------------------------------------------------------------------------------------
    def _check_batch(self, s, a, r, s2, mask, noise):
        dev = self.device
        for t, cols, what in ((s, 10, "state"), (a, 2, "action"), (s2, 10, "next_state")):
            rows2(t, cols, dev, what, unit_stride=False)
        rows = s.shape[0]
        if rows < 1 or a.shape[0] != rows or s2.shape[0] != rows:
            raise ValueError(f"uavx: state, action and next_state must have the same B >= 1 rows, got {rows}, "
                             f"{a.shape[0]}, {s2.shape[0]}")
        for t, what in ((r, "reward"), (mask, "mask")):
            column(t, rows, dev, what)
        if self._noises == 0:
            if noise is not None:
                raise ValueError(f"uavx: {type(self).__name__} draws no noise in its update")
            return rows, ()
        if noise is None:
            return rows, (None,) * self._noises
        noise = (noise,) if torch.is_tensor(noise) else tuple(noise)
        if len(noise) != self._noises:
            raise ValueError(f"uavx: {type(self).__name__}.update_batch takes {self._noises} noise tensor(s) "
                             f"([B, 2] standard normal), got {len(noise)}")
        for n in noise:
            check_f32(n, dev, "noise")
            if tuple(n.shape) != (rows, 2) or not n.is_contiguous():
                raise ValueError(f"uavx: noise must be a contiguous [{rows}, 2] tensor, got {tuple(n.shape)}")
        return rows, noise

    def _target_out(self, rows):
        """y [rows, 1]: the reserved buffer, or a new one outside a capture."""
        if self._y is not None and self._y.shape[0] >= rows:
            return self._y[:rows]
        capture_guard("buffers", rows)
        return torch.empty((rows, 1), dtype=torch.float32, device=self.device)

    def reserve(self, rows):
        """Sizes every workspace and buffer an update of `rows` rows needs (a graph capture cannot allocate them)."""
        rows = int(rows)
        closs, pgrad = self._pieces()
        closs.reserve(rows)
        pgrad.reserve(rows)
        if self._y is None or self._y.shape[0] < rows:
            self._y = torch.empty((rows, 1), dtype=torch.float32, device=self.device)
        if self._sampler is not None:
            self._sampler.reserve(rows)
        if self.prioritized is not None:
            self._q_out(rows)
        return self

    def update_batch(self, s, a, r, s2, mask, noise=None, updates=None, key=None, weight=None):
        """One update of the reference's update_parameters on the given device tensors: state [B, 10], action [B, 2],
        reward and mask [B] or [B, 1], next_state [B, 10].  noise: the standard-normal draws of the update as [B, 2] device
        tensors -- SAC (target's, policy's), TD3 the target's, DDPG none; None draws them from the learner's generator.
        updates: the reference's `updates` argument (TD3's policy_freq, SAC's target_update_interval); None = the number of
        updates run so far.  key: the [B] int64 keys a PrioritizedReplaySampler returned with the batch: the update then
        feeds |q - y| back as their priorities; None leaves the priorities alone.  weight: importance-sampling weights
        ([B] or [B, 1] float32, finite and >= 0, e.g. the sampler's) that multiply each row's critic loss (§24); a weight
        without a key weights the loss and leaves the priorities alone.  Returns nothing: the numbers are in the loss ring
        (losses())."""
        rows, noise = self._check_batch(s, a, r, s2, mask, noise)
        if key is not None:
            self._check_key(key, rows)
        if weight is not None and column(weight, rows, self.device, "weight") < 1:
            raise ValueError("uavx: weight must have a positive row stride")
        u = self.updates if updates is None else int(updates)
        self._update(s, a, r, s2, mask, noise, self._full(u), None if key is None else (key, False), weight)
        self.updates += 1

    def _discount(self):
        return self.gamma

    def attach(self, memory):
        """The DeviceReplay that update_parameters(None, ...) and capture() sample from: through a FusedReplaySampler, or,
        for a learner built with n_step > 1 or recency > 0, through an NStepReplaySampler with the learner's discount, or,
        for one built with prioritized=alpha, through a PrioritizedReplaySampler with beta = per_beta (0: every weight is
        1 and the update does not read them) -- with per_n_step > 1 through a PrioritizedNStepSampler, which walks that many
        steps from each drawn transition with the learner's discount (§25)."""
        if not isinstance(memory, DeviceReplay):
            raise TypeError(f"uavx: the learners sample from a DeviceReplay, not {type(memory).__name__}")
        if self.memory is not memory:
            if self.prioritized is not None and self.per_n_step > 1:      # the walk discounts with the learner's discount
                sampler = PrioritizedNStepSampler(memory, alpha=self.prioritized, beta=self.per_beta, eps=self.per_eps,
                                                  n_step=self.per_n_step, gamma=self._discount())
            elif self.prioritized is not None:
                sampler = PrioritizedReplaySampler(memory, alpha=self.prioritized, beta=self.per_beta, eps=self.per_eps)
            elif self.n_step == 1 and self.recency == 0.0:
                sampler = FusedReplaySampler(memory)
            else:           # the walk discounts with the learner's own discount, so that y = R + discount^len * mask' * (...)
                sampler = NStepReplaySampler(memory, n_step=self.n_step, gamma=self._discount(), recency=self.recency)
            self.memory, self._sampler = memory, sampler
            self._graphs = None
        return self

    def update_parameters(self, memory, batch_size, updates=None):
        """One update, eager, with no host synchronisation.  memory: a DeviceReplay (sampled through FusedReplaySampler
        with the learner's generator), None for the attached one, or an explicit (state, action, reward, next_state, mask)
        tuple of device tensors.  Returns nothing: the numbers are in the loss ring."""
        if isinstance(memory, (tuple, list)):
            if len(memory) != 5:
                raise ValueError(f"uavx: an explicit batch is (state, action, reward, next_state, mask), got {len(memory)} "
                                 f"entries")
            s, a, r, s2, mask = memory
            if s.shape[0] != int(batch_size):
                raise ValueError(f"uavx: the batch has {s.shape[0]} rows, batch_size is {batch_size}")
        else:
            if memory is not None:
                self.attach(memory)
            if self._sampler is None:
                raise ValueError("uavx: update_parameters needs a DeviceReplay (or attach() one first)")
            batch = self._sampler.sample(int(batch_size), generator=self.generator)
            if self.prioritized is not None:         # (..., weight, key): with per_beta == 0 the weight is 1 and not read
                self.update_batch(*batch[:5], updates=updates, key=batch[6],
                                  weight=batch[5] if self._per_weighted else None)
                return
            s, a, r, s2, mask = batch
        self.update_batch(s, a, r, s2, mask, updates=updates)

    # ---- capture / run ------------------------------------------------------------------------------------------------
    def _throwaway(self):
        """A learner of the same class and shapes whose one update loads every kernel before a capture."""
        raise NotImplementedError

    def capture(self, batch_size, memory=None):
        """Captures one update of `batch_size` rows, sampling included, as a torch.cuda.graph (TD3: two, critic-only and
        full; SAC with target_update_interval > 1: two, with and without the target update).  The graph samples from the
        attached DeviceReplay (`memory` attaches one) with the learner's generator and reads the ring's fill through a
        device count that run() refreshes."""
        rows = int(batch_size)
        if rows < 1:
            raise ValueError(f"uavx: capture needs batch_size >= 1, got {batch_size}")
        if memory is not None:
            self.attach(memory)
        if self._sampler is None:
            raise ValueError("uavx: capture needs a DeviceReplay: pass memory= here or to the constructor")
        dev, gen, sampler = self.device, self.generator, self._sampler
        self.reserve(rows)
        # everything a first call creates lazily happens here, on a side stream: the kernels are loaded by a throw-away
        # learner's update, the sampler's uniforms by a sample whose draw is taken back
        state = None if gen is None else gen.get_state()
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.random.fork_rng(devices=[dev]), torch.cuda.stream(side):
            batch = sampler.sample(rows, generator=gen)
            warm = self._throwaway()
            for full in self._variants():
                warm._update(*batch[:5], (None,) * self._noises, full)
            if self._per_weighted:                   # the weighted gradient's kernels, into the throw-away critic's .grad,
                y = self._target_out(rows)           # and the feedback's on keys of -1: nothing is written
                q = self._q_out(rows)[0]
                warm._closs.backward(batch[0], batch[1], y, weight=batch[5], q_out=q)
                sampler.update_priorities(sampler._none[rows], q, y)
            elif self.prioritized is not None:       # the feedback's kernels, on keys of -1: nothing is written
                self._feedback(batch[0], batch[1], self._target_out(rows), (sampler._none[rows], False))
            torch.cuda.synchronize(dev)
            warm.close()
        torch.cuda.current_stream(dev).wait_stream(side)
        if gen is not None:
            gen.set_state(state)
        self._batch = tuple(torch.empty_like(t) for t in batch)
        graphs = {}
        for full in self._variants():
            g = torch.cuda.CUDAGraph()
            if gen is not None:
                g.register_generator_state(gen)
            with torch.cuda.graph(g):
                b = sampler.sample(rows, generator=gen, out=self._batch, device_count=True)
                self._update(*b[:5], (None,) * self._noises, full, (b[6], True) if self.prioritized is not None else None,
                             b[5] if self._per_weighted else None)
            graphs[full] = g
        self._graphs = graphs
        return self

    def run(self, n=1):
        """Replays the captured update n times (no host synchronisation)."""
        if self._graphs is None:
            raise RuntimeError("uavx: run() needs capture(batch_size) first")
        for _ in range(int(n)):
            self._sampler.push_count()
            self._graphs[self._full(self.updates)].replay()
            self._ran(self._full(self.updates))
            self.updates += 1

    def _ran(self, full):
        """Host bookkeeping behind a replay."""

    # ---- reading back -------------------------------------------------------------------------------------------------
    def losses(self, last=None):
        """The last `last` rows of the loss ring (None: all it still holds) in update order, as a numpy [n, 8] array: the
        one host read (a single device-to-host copy of the ring and its count; it synchronises)."""
        return self._rows(self._ring.cpu(), last)

    def _rows(self, ring, last):
        size = self.log_capacity * LOG_COLUMNS
        u, log = int(ring[size:size + 2].view(torch.int64)), ring[:size].view(self.log_capacity, LOG_COLUMNS).numpy()
        n = min(u, self.log_capacity) if last is None else min(int(last), u, self.log_capacity)
        return log[[(u - n + i) % self.log_capacity for i in range(n)]].reshape(n, LOG_COLUMNS)

    def report(self, last=None):
        """losses(last) and, from the SAME host read, the clip records (§26): (rows, {"critic": (grad_norm, clip_coef,
        clipped_steps), "actor": (...)}) as Python numbers, None for an optimiser that does not clip."""
        ring = self._ring.cpu()
        off = self.log_capacity * LOG_COLUMNS + 2
        norms = {}
        for k, name in enumerate(("critic", "actor")):
            rec = ring[off + k * _CLIP_RECORD:off + (k + 1) * _CLIP_RECORD]
            norms[name] = None if self.max_grad_norm[k] is None else (float(rec[0]), float(rec[1]),
                                                                      int(rec[2:4].view(torch.int64)))
        return self._rows(ring, last), norms

    def _set_updates(self, u):
        self.updates = int(u)
        self._updates.fill_(self.updates)

    def exploration(self, memory_or_rows, **kw):
        """An Exploration (exploration.py) bound to the packed actor select_action acts with.
        memory_or_rows: a DeviceReplay (every agent of every env acts: num_envs * num_agents rows; the ring is kept for
        reset_on_episode) or the number of acting rows.  kw: Exploration's arguments; a learner's own noise scale is the
        default (DDPG's ou_sigma = noise_std_dev, TD3's noise_std = 0.1)."""
        from .exploration import Exploration
        memory = None if isinstance(memory_or_rows, int) else memory_or_rows
        rows = memory_or_rows if memory is None else memory.env.num_envs * memory.env.num_agents
        for k, v in self._explore_defaults().items():
            kw.setdefault(k, v)
        ex = Exploration(self._actor_h, rows, **kw)
        ex.memory = memory
        return ex

    def _explore_defaults(self):
        return {}

    def _explore(self, actor, explore, obs, out):
        if explore.actor is not actor:
            raise ValueError("uavx: this Exploration is bound to another actor; build it with this learner's exploration()")
        return explore.act(obs, out=out)

    def refresh(self):
        """Re-packs every snapshot the kernels read: call it after writing into the modules by hand (load_state_dict);
        load_checkpoint does it itself."""
        for h in self._packed():
            h.refresh()
        return self

    # ---- the whole learner, for a run that stops and continues (checkpoint.py) ---------------------------
    def _nets(self):
        """{attribute name: module} of every network and target."""
        raise NotImplementedError

    def _optims(self):
        """{attribute name of the torch optimiser: its FusedAdam}."""
        raise NotImplementedError

    def _config_extra(self):
        return {}

    def _config(self):
        """What a saved learner must share with the one it is loaded into: checked by load_state_dict, never applied."""
        cfg = {"class": type(self).__name__, "dims": dict(self._dims), "log_capacity": self.log_capacity,
               "n_step": self.n_step, "recency": self.recency, "prioritized": self.prioritized, "per_eps": self.per_eps,
               "per_n_step": self.per_n_step, "weighted": self._per_weighted,
               "clips": [a.max_grad_norm is not None for a in self._adams()]}
        cfg.update(self._config_extra())
        return cfg

    def state_dict(self, include_sampler=True):
        """Everything a bit-exact continuation of this learner needs, on the CPU, as tensors and built-in types: the
        modules, the optimisers' state (device step counts synced first, as save_checkpoint does), `updates`, the whole
        loss-ring allocation (loss rows, the device update count, both clip records with their bounds), per_beta,
        max_grad_norm, the attached prioritized sampler's state (include_sampler=False leaves it out; the uniform and
        n-step samplers have none) and the configuration load_state_dict validates.  It synchronises: keep it out of the
        update loop."""
        optims = self._optims()
        for adam in optims.values():
            adam.sync_state()
        sampler = None
        if include_sampler and isinstance(self._sampler, PrioritizedReplaySampler):
            sampler = self._sampler.state_dict()
        return {"config": self._config(),
                "modules": {name: _cpu(m.state_dict()) for name, m in self._nets().items()},
                "optimizers": {name: _cpu(adam.optimizer.state_dict()) for name, adam in optims.items()},
                "updates": int(self.updates), "ring": self._ring.detach().cpu().clone(), "per_beta": float(self.per_beta),
                "max_grad_norm": list(self.max_grad_norm), "sampler": sampler}

    def _check_state(self, sd):
        """Refuses a state_dict() this learner cannot continue, naming the field, before load_state_dict writes anything."""
        who, mine = type(self).__name__, self._config()
        saved = sd.get("config")
        if not isinstance(saved, dict):
            raise ValueError(f"uavx: {who}.load_state_dict takes a learner's state_dict(): no configuration block")
        for field in ("class",) + tuple(k for k in mine if k != "class"):
            if field not in saved or saved[field] != mine[field]:
                raise ValueError(f"uavx: the saved learner has {field} = {saved.get(field)!r}, this {who} {field} = "
                                 f"{mine[field]!r}")
        for part, names in (("modules", self._nets()), ("optimizers", self._optims())):
            if not isinstance(sd.get(part), dict) or set(sd[part]) != set(names):
                raise ValueError(f"uavx: the saved learner's {part} are {sorted(sd.get(part) or ())}, this {who}'s "
                                 f"{sorted(names)}")
        ring = sd.get("ring")
        if not torch.is_tensor(ring) or ring.dtype != torch.float32 or tuple(ring.shape) != tuple(self._ring.shape):
            raise ValueError(f"uavx: the saved loss ring does not have this {who}'s {tuple(self._ring.shape)} float32 layout")
        self._check_per_beta(sd["per_beta"])
        self._check_max_grad_norm(sd["max_grad_norm"])
        if sd.get("sampler") is not None:
            if not isinstance(self._sampler, PrioritizedReplaySampler):
                raise ValueError(f"uavx: the saved learner carries a priority table: attach() a DeviceReplay to this {who} "
                                 f"before loading it")
            table = sd["sampler"]["table"]
            if tuple(table.shape) != tuple(self._sampler._table.shape):
                raise ValueError(f"uavx: the saved priority table is {tuple(table.shape)}, this ring's "
                                 f"{tuple(self._sampler._table.shape)}")

    def _load_extra(self, sd):
        """What a subclass keeps besides modules and optimisers."""

    def load_state_dict(self, sd):
        """Restores a state_dict() of a learner of the same class and configuration.  A mismatch is refused with a message
        that names the field, before anything is written.  Parameters, the loss ring and the sampler's table are written
        in place; every fused handle is re-packed, and captured graphs are dropped (they hold the addresses of the optimiser
        state this call replaced): capture() again before run()."""
        self._check_state(sd)
        for name, m in self._nets().items():
            m.load_state_dict(sd["modules"][name])
        for name, adam in self._optims().items():
            adam.load_state_dict(sd["optimizers"][name])
        self._load_extra(sd)
        self._ring.copy_(sd["ring"])
        self.updates = int(sd["updates"])
        if self._per_weighted:
            self.set_per_beta(sd["per_beta"])
        if any(b is not None for b in sd["max_grad_norm"]):
            self.set_max_grad_norm(tuple(sd["max_grad_norm"]))
        if sd.get("sampler") is not None:
            self._sampler.load_state_dict(sd["sampler"])
        self._graphs = None
        return self._repack()

    def _repack(self):
        return self.refresh()

    def close(self):
        for x in self._handles():
            x.close()


class FusedSAC(_FusedLearner):
    """sac.py's SAC: policy, critic, critic_target, critic_optim, policy_optim, log_alpha, alpha_optim under the
    reference's names; `alpha` is the 1-element device tensor every kernel reads."""
    kind = _actor_lib.SAC
    _noises = 2

    def __init__(self, n_states=10, n_actions=2, lr=3e-4, tau=5e-3, gamma=0.99, alpah=2, target_update_interval=1,
                 automatic_entropy_tuning=True, target_entropy=None, device="cuda", generator=None, log_capacity=1024,
                 memory=None, hidden=256, n_step=1, recency=0.0, prioritized=None, per_eps=1e-6, per_beta=0.0, per_n_step=1,
                 max_grad_norm=None):
        self.lr, self.tau, self.gamma = lr, tau, gamma
        self.target_update_interval = int(target_update_interval)
        if self.target_update_interval < 1:
            raise ValueError(f"uavx: target_update_interval must be >= 1, got {target_update_interval}")
        self.automatic_entropy_tuning = bool(automatic_entropy_tuning)
        self._setup(device, generator, log_capacity, memory, n_step, recency, prioritized, per_eps, per_beta, per_n_step,
                    max_grad_norm)
        dev = self.device
        self._dims = dict(n_states=n_states, n_actions=n_actions, hidden=hidden)
        self.critic = policy.TwinQ(n_states, n_actions, hidden).to(dev)
        self.critic_optim = torch.optim.Adam(self.critic.parameters(), lr=lr)
        self.critic_target = policy.TwinQ(n_states, n_actions, hidden).to(dev)
        _copy_params(self.critic_target, self.critic)                                  # hard_update, sac.py:26
        self._alpha = torch.full((1,), float(alpah), dtype=torch.float32, device=dev)  # update 0 runs with `alpah`
        self.target_entropy = -float(n_actions) if target_entropy is None else float(target_entropy)
        if self.automatic_entropy_tuning:
            self.log_alpha = torch.zeros(1, requires_grad=True, device=dev)
            self.alpha_optim = torch.optim.Adam([self.log_alpha], lr=lr)
            self._alpha_adam = FusedAdam(self.alpha_optim)      # keeps the state in torch's format; the tail does the step
        self.policy = policy.GaussianPolicy(n_states, n_actions, hidden).to(dev)
        with torch.no_grad():
            for m in self.policy.modules():                                             # weights_init_, model.py:10-14
                if isinstance(m, torch.nn.Linear):
                    torch.nn.init.xavier_uniform_(m.weight, gain=1)
                    torch.nn.init.constant_(m.bias, 0)
        self.policy_optim = torch.optim.Adam(self.policy.parameters(), lr=lr)
        self._build()

    def _build(self):
        # the target block reads packed snapshots of the LIVE policy (sac.py:57) and of critic_target
        self._actor_h = FusedActor.from_module(self.policy)
        self._target_h = FusedCritic.from_module(self.critic_target)
        self._target = FusedTarget(self._actor_h, self._target_h, gamma=self.gamma)
        self._closs = FusedCriticLoss(self.critic)
        self._pgrad = FusedPolicyGrad(self.policy, self._closs.critic)
        self._critic_adam = FusedAdam(self.critic_optim, target=self.critic_target, tau=self.tau, **self._clip_kw(0))
        self._policy_adam = FusedAdam(self.policy_optim, **self._clip_kw(1))

    def _adams(self):
        return (self._critic_adam, self._policy_adam)

    def _handles(self):
        return (self._pgrad, self._closs, self._target, self._actor_h, self._target_h)

    def _packed(self):
        return (self._actor_h, self._target_h)

    def _nets(self):
        return {"policy": self.policy, "critic": self.critic, "critic_target": self.critic_target}

    def _optims(self):
        out = {"critic_optim": self._critic_adam, "policy_optim": self._policy_adam}
        if self.automatic_entropy_tuning:
            out["alpha_optim"] = self._alpha_adam
        return out

    def _config_extra(self):
        return {"automatic_entropy_tuning": self.automatic_entropy_tuning,
                "target_update_interval": self.target_update_interval}

    def state_dict(self, include_sampler=True):
        sd = super().state_dict(include_sampler)
        sd["alpha"] = self._alpha.detach().cpu().clone()
        if self.automatic_entropy_tuning:
            sd["log_alpha"] = self.log_alpha.detach().cpu().clone()
        return sd

    def _check_state(self, sd):
        super()._check_state(sd)
        for name in ("alpha",) + (("log_alpha",) if self.automatic_entropy_tuning else ()):
            t = sd.get(name)
            if not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != (1,):
                raise ValueError(f"uavx: the saved learner's {name} must be a float32 tensor of one element")

    def _load_extra(self, sd):
        self._alpha.copy_(sd["alpha"])
        if self.automatic_entropy_tuning:
            with torch.no_grad():
                self.log_alpha.copy_(sd["log_alpha"])

    @property
    def alpha(self):
        """The temperature the next update runs with: a 1-element float32 device tensor."""
        return self._alpha

    def _variants(self):
        return (True,) if self.target_update_interval == 1 else (True, False)

    def _full(self, updates):
        return updates % self.target_update_interval == 0

    def _update(self, s, a, r, s2, mask, noise, full, key=None, weight=None):
        gen = self.generator
        y = self._target(s2, r, mask, alpha=self._alpha, generator=gen, noise=noise[0], out=self._target_out(s.shape[0]))
        critic_loss = self._critic_grad(s, a, y, key, weight)
        # the soft update reads only the critic: it rides in the critic's step, and the packed target follows it
        self._critic_adam.step(update_target=full, refresh=self._target_h if full else None)
        policy_loss, _ = self._pgrad.backward(s, alpha=self._alpha, noise=noise[1], generator=gen)
        self._policy_adam.step(refresh=self._actor_h)
        sac = None
        if self.automatic_entropy_tuning:
            sac = (self._pgrad.log_pi_mean, self._alpha_adam.hyper())
        self._tail(critic_loss, policy_loss, sac)

    def _throwaway(self):
        return FusedSAC(lr=self.lr, tau=self.tau, gamma=self.gamma, device=self.device, log_capacity=1,
                        automatic_entropy_tuning=self.automatic_entropy_tuning, max_grad_norm=self.max_grad_norm,
                        **self._dims)

    def select_action(self, obs, evaluate=False, out=None, explore=None):
        """sac.py:38-44 over any batch of observations [..., 10] on the device: tanh(mean + std·eps), or tanh(mean) when
        evaluating; one launch on the packed live policy.  explore: an Exploration of this learner (exploration()): the
        trainer's acting step with warm-up, random actions and Philox noise instead, two launches; `evaluate` is not read."""
        if explore is not None:
            return self._explore(self._actor_h, explore, obs, out)
        return self._actor_h.act(obs, evaluate=evaluate, generator=self.generator, out=out)

    def save_checkpoint(self, ckpt_path, file_name=None):
        """sac.py:101-114's file (policy.save_reference_checkpoint), plus what a bit-exact continuation needs and the
        reference does not keep: log_alpha, its optimiser, alpha and the update count."""
        path = os.path.join(ckpt_path, "weights.chpt" if file_name is None else file_name)
        self._critic_adam.sync_state()
        self._policy_adam.sync_state()
        policy.save_reference_checkpoint(path, self.policy, self.critic, self.critic_target, self.critic_optim,
                                         self.policy_optim)
        extra = {"alpha": self._alpha.detach().cpu(), "updates": self.updates}
        if self.automatic_entropy_tuning:
            extra["log_alpha"] = self.log_alpha.detach().cpu()
            extra["alpha_optimizer_state_dict"] = _cpu(self._alpha_adam.state_dict())
        _amend(path, extra)
        return path

    def load_checkpoint(self, ckpt_path, file_name=None, evaluate=False):
        path = os.path.join(ckpt_path, "weights.chpt" if file_name is None else file_name)
        ck = torch.load(path, map_location=self.device, weights_only=True)
        self.policy.load_state_dict(ck["policy_state_dict"])
        self.critic.load_state_dict(ck["critic_state_dict"])
        self.critic_target.load_state_dict(ck["critic_target_state_dict"])
        self._critic_adam.load_state_dict(ck["critic_optimizer_state_dict"])
        self._policy_adam.load_state_dict(ck["policy_optimizer_state_dict"])
        if "alpha" in ck:
            self._alpha.copy_(ck["alpha"])
        if self.automatic_entropy_tuning and "log_alpha" in ck:
            with torch.no_grad():
                self.log_alpha.copy_(ck["log_alpha"])
            self._alpha_adam.load_state_dict(ck["alpha_optimizer_state_dict"])
        self._set_updates(ck.get("updates", 0))
        for m in (self.policy, self.critic, self.critic_target):
            m.eval() if evaluate else m.train()
        self._graphs = None                 # a captured graph holds the addresses of the optimiser state it replaced
        return self.refresh()


class _ActorCriticLearner(_FusedLearner):
    """TD3 and DDPG: actor, actor_target, critic, critic_target and the two optimisers."""

    def _build(self, **target_kw):
        self._actor_h = FusedActor.from_module(self.actor)          # select_action's: the live actor (_live)
        self._stale = False
        self._target = FusedTarget(self.actor_target, self.critic_target, gamma=self._gamma, **target_kw)
        self._closs = FusedCriticLoss(self.critic)
        self._pgrad = FusedPolicyGrad(self.actor, self._closs.critic)
        self._critic_adam = FusedAdam(self.critic_optimizer, **self._clip_kw(0))
        self._actor_adam = FusedAdam(self.actor_optimizer, target=self.actor_target, tau=self.tau, **self._clip_kw(1))

    def _adams(self):
        return (self._critic_adam, self._actor_adam)

    def _handles(self):
        return (self._pgrad, self._closs, self._target, self._actor_h)

    def _packed(self):
        return (self._actor_h, self._target)

    def _nets(self):
        return {"actor": self.actor, "actor_target": self.actor_target, "critic": self.critic,
                "critic_target": self.critic_target}

    def _optims(self):
        return {"critic_optimizer": self._critic_adam, "actor_optimizer": self._actor_adam}

    def _repack(self):
        self.refresh()                      # select_action's lazily re-packed actor included: it is current now
        self._stale = False
        return self

    def _actor_and_targets(self, s):
        """The actor update and both soft updates, the actor's first (td3.py:141-156, ddpg.py:73-83) -> the actor loss."""
        actor_loss = self._pgrad.backward(s)
        self._actor_adam.step(update_target=True)
        soft_update(self.critic_target, self.critic, self.tau)
        self._target.refresh()
        self._stale = True
        return actor_loss

    def _ran(self, full):
        self._stale = self._stale or full

    def refresh_actor(self):
        """Re-packs select_action's copy of the live actor now (one launch on the current stream).  select_action does it
        itself when an actor step was enqueued since the last re-pack; call this before capturing select_action in a
        graph of your own, and inside that graph behind the learner's update if the graph holds both."""
        self._actor_h.refresh()
        self._stale = False
        return self

    def _live(self):
        """select_action's packed actor.  No update reads it, so it is re-packed here, behind the actor steps enqueued since
        the last call, rather than by a launch in every update."""
        if self._stale:
            self.refresh_actor()
        return self._actor_h

    def _load_modules(self, actor_ck, critic_ck, keys):
        a, at, c, ct, ao, co = keys
        self.actor.load_state_dict(actor_ck[a])
        self.actor_target.load_state_dict(actor_ck[at])
        self.critic.load_state_dict(critic_ck[c])
        self.critic_target.load_state_dict(critic_ck[ct])
        self._actor_adam.load_state_dict(actor_ck[ao])
        self._critic_adam.load_state_dict(critic_ck[co])
        self._set_updates(actor_ck.get("updates", 0))
        self._graphs = None                 # a captured graph holds the addresses of the optimiser state it replaced
        self.refresh()


class FusedTD3(_ActorCriticLearner):
    """td3.py's TD3 under the reference's attribute names; lr = 3e-4 on both optimisers (td3.py:81,85)."""
    kind = _actor_lib.TD3
    _noises = 1

    def __init__(self, state_dim=10, action_dim=2, discount=0.99, tau=0.005, policy_noise=0.2, noise_clip=0.5,
                 policy_freq=2, device="cuda", generator=None, log_capacity=1024, memory=None, hidden=256, n_step=1,
                 recency=0.0, prioritized=None, per_eps=1e-6, per_beta=0.0, per_n_step=1, max_grad_norm=None):
        self.discount, self.tau, self.policy_noise, self.noise_clip = discount, tau, policy_noise, noise_clip
        self.policy_freq = int(policy_freq)
        if self.policy_freq < 1:
            raise ValueError(f"uavx: policy_freq must be >= 1, got {policy_freq}")
        self.max_action = 1
        self._setup(device, generator, log_capacity, memory, n_step, recency, prioritized, per_eps, per_beta, per_n_step,
                    max_grad_norm)
        dev = self.device
        self._dims = dict(state_dim=state_dim, action_dim=action_dim, hidden=hidden)
        self.actor = policy.TD3Actor(state_dim, action_dim, hidden).to(dev)
        self.actor_target = policy.TD3Actor(state_dim, action_dim, hidden).to(dev)
        _copy_params(self.actor_target, self.actor)                                    # copy.deepcopy, td3.py:80
        self.actor_optimizer = torch.optim.Adam(self.actor.parameters(), lr=3e-4)
        self.critic = policy.TD3TwinQ(state_dim, action_dim, hidden).to(dev)
        self.critic_target = policy.TD3TwinQ(state_dim, action_dim, hidden).to(dev)
        _copy_params(self.critic_target, self.critic)
        self.critic_optimizer = torch.optim.Adam(self.critic.parameters(), lr=3e-4)
        self._gamma = discount
        self._build(policy_noise=policy_noise, noise_clip=noise_clip)

    def _discount(self):
        return self.discount

    def _config_extra(self):
        return {"policy_freq": self.policy_freq}

    def _variants(self):
        return (True,) if self.policy_freq == 1 else (True, False)

    def _full(self, updates):
        return updates % self.policy_freq == 0

    def _update(self, s, a, r, s2, mask, noise, full, key=None, weight=None):
        y = self._target(s2, r, mask, generator=self.generator, noise=noise[0], out=self._target_out(s.shape[0]))
        critic_loss = self._critic_grad(s, a, y, key, weight)
        self._critic_adam.step(update_target=False)
        self._tail(critic_loss, self._actor_and_targets(s) if full else None)

    def _throwaway(self):
        return FusedTD3(device=self.device, log_capacity=1, max_grad_norm=self.max_grad_norm, **self._dims)

    def _explore_defaults(self):
        return {"noise_std": 0.1}

    def select_action(self, obs, evaluate=True, noise_std=0.1, out=None, explore=None):
        """td3.py:95-97 over any batch of observations [..., 10] on the device; evaluate=False adds the trainer's clipped
        Gaussian exploration noise (FusedActor.act).  The packed actor is re-packed by this call when an
        actor step was enqueued since the last re-pack (a host flag): a capture of this call alone bakes in that re-pack or
        its absence, so call refresh_actor() explicitly around captures of your own.  explore: an Exploration of this learner
        (exploration()): the same re-pack, then the trainer's acting step with warm-up, random actions and Philox noise;
        `evaluate` and `noise_std` are not read."""
        if explore is not None:
            return self._explore(self._live(), explore, obs, out)
        return self._live().act(obs, evaluate=evaluate, generator=self.generator, noise_std=noise_std, out=out)

    def save_checkpoint(self, ckpt_path, file_name=None):
        """td3.py:159-170's file (policy.save_td3_checkpoint) with the targets as they are, plus the update count."""
        path = os.path.join(ckpt_path, "weights.chpt" if file_name is None else file_name)
        self._actor_adam.sync_state()
        self._critic_adam.sync_state()
        policy.save_td3_checkpoint(path, self.actor, self.critic, self.actor_optimizer, self.critic_optimizer)
        _amend(path, {"actor_target_state_dict": _cpu(self.actor_target.state_dict()),
                      "critic_target_state_dict": _cpu(self.critic_target.state_dict()),
                      "updates": self.updates})
        return path

    def load_checkpoint(self, ckpt_path, file_name=None):
        path = os.path.join(ckpt_path, "weights.chpt" if file_name is None else file_name)
        ck = torch.load(path, map_location=self.device, weights_only=True)
        self._load_modules(ck, ck, policy.TD3_CHECKPOINT_KEYS)
        return self


class FusedDDPG(_ActorCriticLearner):
    """ddpg.py's DDPG under the reference's attribute names: AMSGrad on both optimisers, an L1 critic loss."""
    kind = _actor_lib.DDPG
    _noises = 0

    def __init__(self, n_states=10, n_actions=2, noise_std_dev=0.2, actor_lr=1e-4, critic_lr=1e-3, tau=5e-3, gamma=0.99,
                 device="cuda", generator=None, log_capacity=1024, memory=None, hidden1=400, hidden2=300, n_step=1,
                 recency=0.0, prioritized=None, per_eps=1e-6, per_beta=0.0, per_n_step=1, max_grad_norm=None):
        self.n_states, self.n_actions = n_states, n_actions
        self.noise_std_dev, self.tau, self.gamma = float(noise_std_dev), tau, gamma
        self._setup(device, generator, log_capacity, memory, n_step, recency, prioritized, per_eps, per_beta, per_n_step,
                    max_grad_norm)
        dev = self.device
        self._dims = dict(n_states=n_states, n_actions=n_actions, hidden1=hidden1, hidden2=hidden2)
        self.actor = ddpg_init(policy.DDPGActor(n_states, n_actions, hidden1, hidden2), 5e-4).to(dev)     # model.py:8,19-22
        self.actor_target = policy.DDPGActor(n_states, n_actions, hidden1, hidden2).to(dev)
        self.actor_optimizer = torch.optim.Adam(self.actor.parameters(), lr=actor_lr, amsgrad=True)
        self.critic = ddpg_init(policy.DDPGCritic(n_states, n_actions, hidden1, hidden2), 5e-5).to(dev)   # model.py:38,48-51
        self.critic_target = policy.DDPGCritic(n_states, n_actions, hidden1, hidden2).to(dev)
        self.critic_optimizer = torch.optim.Adam(self.critic.parameters(), lr=critic_lr, amsgrad=True)
        _copy_params(self.actor_target, self.actor)                                    # _hard_update, ddpg.py:27-28
        _copy_params(self.critic_target, self.critic)
        self._gamma = gamma
        self._build()

    def _update(self, s, a, r, s2, mask, noise, full, key=None, weight=None):
        y = self._target(s2, r, mask, out=self._target_out(s.shape[0]))
        critic_loss = self._critic_grad(s, a, y, key, weight)
        self._critic_adam.step(update_target=False)
        self._tail(critic_loss, self._actor_and_targets(s))

    def _throwaway(self):
        return FusedDDPG(device=self.device, log_capacity=1, max_grad_norm=self.max_grad_norm, **self._dims)

    def _explore_defaults(self):
        return {"ou_sigma": self.noise_std_dev}

    def select_action(self, obs, evaluate=False, noise=None, out=None, explore=None):
        """ddpg.py:39-47 over any batch of observations [..., 10] on the device.  evaluate=False adds `noise` (the caller's
        Ornstein-Uhlenbeck state, a tensor broadcastable to the actions) and clips to [-1, 1].  The packed actor is re-packed by this call when an
        actor step was enqueued since the last re-pack (a host flag): a capture of this call alone bakes in that re-pack or
        its absence, so call refresh_actor() explicitly around captures of your own.  explore: an Exploration of this learner
        (exploration()): the same re-pack, then the OU process kept on the device, with warm-up and random actions;
        `evaluate` and `noise` are not read."""
        if explore is not None:
            return self._explore(self._live(), explore, obs, out)
        return self._live().act(obs, evaluate=evaluate, noise=noise, out=out)

    def save_checkpoint(self, output):
        """ddpg.py:124-135's actor.chpt and critic.chpt in the directory `output` (policy.save_ddpg_checkpoint) with the
        targets as they are, plus the update count."""
        self._actor_adam.sync_state()
        self._critic_adam.sync_state()
        policy.save_ddpg_checkpoint(output, self.actor, self.critic, self.actor_optimizer, self.critic_optimizer)
        _amend(os.path.join(output, "actor.chpt"), {"target_model_state_dict": _cpu(self.actor_target.state_dict()),
                                                    "updates": self.updates})
        _amend(os.path.join(output, "critic.chpt"),
               {"target_model_state_dict": _cpu(self.critic_target.state_dict())})
        return output

    def load_checkpoint(self, output):
        ack = torch.load(os.path.join(output, "actor.chpt"), map_location=self.device, weights_only=True)
        cck = torch.load(os.path.join(output, "critic.chpt"), map_location=self.device, weights_only=True)
        m, t, o = policy.DDPG_CHECKPOINT_KEYS
        self._load_modules(ack, cck, (m, t, m, t, o, o))
        return self
