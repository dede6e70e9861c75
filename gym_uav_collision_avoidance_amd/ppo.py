"""PPO on the device ring: the on-policy learner for tens of thousands of parallel worlds.

    mem = DeviceReplay(venv.env, horizon=32)
    mem.begin(venv.reset())
    ppo = PPO(mem, generator=gen)
    for it in range(iterations):
        for _ in range(32):
            ppo.act()                                   # tanh(μ + σ·ε) into the ring's action slot
            mem.step(polar=True, auto_reset="agent0_done", step_cap=1500)
        losses = ppo.update()                           # 0-d device tensors

The rollout IS the ring: act() writes its action into the slot the step launch reads and keeps the pre-squash sample u and
log π(a|s) in two buffers of the ring's shape; update() evaluates the value net over the whole ring in one forward, takes
advantages and returns from rollout.RolloutAdvantages (one HIP walk, libuavx_gae.so) and runs epochs × minibatches steps of
the clipped surrogate.  The networks and their update are plain torch autograd: minibatches of tens of thousands of rows are
the regime where torch's GEMMs are the right tool (README, large-batch figures), so no hand kernel replaces them.

Nothing in update() reads the device from the host, so the set of rows cannot shrink to the valid ones: every (step, env,
learner) row of the window is a row of the batch, and a 0/1 weight takes out what is not a sample -- re-initialisation rows
(valid = 0) and rows of an agent that was already done before the step (parked in an env that went on: the previous row's
done, unless that row ended the episode or was a re-initialisation).  Every mean below is Σ w·x / max(1, Σ w).

fused_heads=True keeps the GEMMs, autograd through the two networks, the clip and Adam in torch and runs what lies between
them in HIP (ppo_heads.PPOHeads, libuavx_ppo.so): act() is the policy's forward, the same torch.randn call and
ONE launch into the slot's u, log π and action; a minibatch is the two forwards, TWO launches that leave the losses and their
gradient with respect to (μ, log σ, V), and torch.autograd.backward from those three.

normalize_obs / normalize_reward keep the running statistics of normalize.RolloutNormalizer (libuavx_norm.so):
the policy and the value net see (obs − mean) / sqrt(var + eps), GAE reads the rewards divided by the standard deviation of
the discounted return.  update() folds the rollout's returns into the record BEFORE it scales the rewards (the scale is
defined from the first update on) and the rollout's observations AFTER its last minibatch: the observation record is frozen
from a rollout's first act() to the end of its update, so the policy that is evaluated is the policy that acted.  Both off
(the default) is the learner without any of it: the library is not loaded and state_dict() has no "norm"."""
import math

import torch

from .policy import GaussianPolicy, ValueNet
from .rollout import RolloutAdvantages

_LOG_2PI = math.log(2.0 * math.pi)
_LOG_2 = math.log(2.0)


def log_prob(mean, log_std, u):
    """log π(tanh(u)) of the tanh-squashed Gaussian, summed over the action dimensions: the Gaussian's log density at u
    minus log|d tanh(u)/du| in its stable form 2·(log 2 − u − softplus(−2u))."""
    z = (u - mean) * torch.exp(-log_std)
    gauss = -0.5 * z * z - log_std - 0.5 * _LOG_2PI
    squash = 2.0 * (_LOG_2 - u - torch.nn.functional.softplus(-2.0 * u))
    return (gauss - squash).sum(-1)


def _positive(name, x, integer=False):
    ok = not isinstance(x, bool) and isinstance(x, int if integer else (int, float)) and x > 0 and math.isfinite(x)
    if not ok:
        raise ValueError(f"uavx: PPO: {name} must be a finite {'int' if integer else 'float'} > 0, got {x!r}")
    return x


class PPO:
    def __init__(self, mem, generator=None, lr=3e-4, gamma=0.99, lam=0.95, clip=0.2, epochs=4, minibatches=4, vf_coef=0.5,
                 ent_coef=0.0, max_grad_norm=0.5, rollout=None, fused_heads=False, normalize_obs=False, normalize_reward=False,
                 clip_obs=10.0, clip_reward=10.0, norm_eps=1e-8):
        """mem: the DeviceReplay the rollout is collected in (its horizon bounds the rollout; num_learners is respected).
        generator: a torch.Generator on the ring's device for the action noise and the minibatch permutations.
        rollout: steps per update, default the ring's horizon.  max_grad_norm: None = no clipping.
        fused_heads: sample and evaluate the losses in HIP (module docstring); not part of state_dict().
        normalize_obs, normalize_reward: keep running statistics and normalise with them (module docstring); clip_obs,
        clip_reward, norm_eps: RolloutNormalizer's clip_obs, clip_reward and eps."""
        for name, x in (("fused_heads", fused_heads), ("normalize_obs", normalize_obs), ("normalize_reward", normalize_reward)):
            if not isinstance(x, bool):
                raise ValueError(f"uavx: PPO: {name} must be a bool, got {x!r}")
        _positive("clip_obs", clip_obs), _positive("clip_reward", clip_reward)
        if isinstance(norm_eps, bool) or not isinstance(norm_eps, (int, float)) or not math.isfinite(norm_eps) or norm_eps < 0:
            raise ValueError(f"uavx: PPO: norm_eps must be a finite float >= 0, got {norm_eps!r}")
        _positive("lr", lr), _positive("clip", clip)
        self.epochs, self.minibatches = _positive("epochs", epochs, True), _positive("minibatches", minibatches, True)
        for name, x in (("vf_coef", vf_coef), ("ent_coef", ent_coef)):
            if isinstance(x, bool) or not isinstance(x, (int, float)) or not math.isfinite(x) or x < 0:
                raise ValueError(f"uavx: PPO: {name} must be a finite float >= 0, got {x!r}")
        if max_grad_norm is not None:
            _positive("max_grad_norm", max_grad_norm)
        self.rollout = mem.T if rollout is None else _positive("rollout", rollout, True)
        if self.rollout > mem.T:
            raise ValueError(f"uavx: PPO: rollout = {self.rollout} steps do not fit the ring's horizon of {mem.T}")
        self.mem, self.generator = mem, generator
        self.clip, self.vf_coef, self.ent_coef, self.max_grad_norm = float(clip), float(vf_coef), float(ent_coef), max_grad_norm
        self.advantages = RolloutAdvantages(mem, gamma=gamma, lam=lam, normalize=True)
        self.device = dev = mem.rew.device
        rows = self.rollout * mem.env.num_envs * mem.num_learners
        if rows % self.minibatches:
            raise ValueError(f"uavx: PPO: {self.minibatches} minibatches do not divide the {rows} rows of a rollout")
        self.policy = GaussianPolicy().to(dev)
        self.value = ValueNet().to(dev)
        self.params = list(self.policy.parameters()) + list(self.value.parameters())
        self.optimizer = torch.optim.Adam(self.params, lr=lr)
        L, E, N = self.advantages.shape
        self.u = torch.zeros((L, E, N, 2), dtype=torch.float32, device=dev)     # pre-squash sample of the slot's action
        self.logp = torch.zeros((L, E, N), dtype=torch.float32, device=dev)     # log π of it under the policy that drew it
        self.updates = 0
        self.values = None            # what the last update() gave RolloutAdvantages
        self.first_ratio = None       # π / π_old over the first minibatch of the last update()'s first epoch
        self.weight = None            # the 0/1 weight of the last update()'s rows, (step oldest first, env, learner) order
        self.fused_heads, self.heads = fused_heads, None
        if fused_heads:
            from .ppo_heads import PPOHeads
            self.heads = PPOHeads(dev)
        self.normalize_obs, self.normalize_reward, self.norm = normalize_obs, normalize_reward, None
        if normalize_obs or normalize_reward:
            from .normalize import RolloutNormalizer
            self.norm = RolloutNormalizer(mem, gamma=gamma, obs=normalize_obs, reward=normalize_reward, clip_obs=clip_obs,
                                          clip_reward=clip_reward, eps=norm_eps)
            self._state = torch.zeros_like(mem.obs[0]) if normalize_obs else None     # what act() shows the policy

    # -- acting --------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def act(self):
        """Samples u = μ + σ·ε for the ring's current state, writes tanh(u) into mem.action_slot() (returned) and keeps u and
        log π at the slot: call mem.step() next."""
        mem = self.mem
        s = mem.count % mem.L
        mean, log_std = self.policy(self.norm.obs(mem.state, out=self._state) if self.normalize_obs else mem.state)
        eps = torch.randn(mean.shape, generator=self.generator, device=mean.device, dtype=mean.dtype)
        if self.fused_heads:
            out = mem.action_slot()
            self.heads.sample(mean, log_std, eps, self.u[s], self.logp[s], out)
            return out
        u = mean + log_std.exp() * eps
        self.u[s].copy_(u)
        self.logp[s].copy_(log_prob(mean, log_std, u))
        out = mem.action_slot()
        torch.tanh(u, out=out)
        return out

    @torch.no_grad()
    def select_action(self, obs, evaluate=True):
        """obs [..., 10] -> actions [..., 2] in [-1, 1] without touching the ring (evaluate.py's policy_fn).  With
        normalize_obs the policy sees the observations normalised by the record as it stands."""
        if self.normalize_obs:
            obs = self.norm.obs(obs.contiguous())
        return self.policy.act(obs, evaluate=evaluate, generator=self.generator)

    # -- learning ------------------------------------------------------------------------------------------------------------
    def _parked(self, slots, first_k):
        """[steps, E, learners] bool: the agent was already done before the step of that row."""
        mem = self.mem
        prev = (slots - 1) % mem.L
        skip, _, ended = mem._flags(prev, slice(None))
        parked = ((mem.done[prev] & 1) != 0) & ~(ended | skip).unsqueeze(-1)
        if first_k == 0:
            parked[0] = False         # the ring's first step has no row before it
        return parked[:, :, :mem.num_learners]

    def update(self):
        """One PPO update over the last `rollout` steps of the ring (fewer while the ring holds fewer).  Returns a dict of 0-d
        device tensors (means over the last epoch's minibatches); nothing is read on the host."""
        mem, nl = self.mem, self.mem.num_learners
        steps = min(self.rollout, mem.count, mem.T)
        if self.normalize_reward:
            self.norm.fold_returns()      # before the rewards are scaled: the scale is defined from the first update on
        ring_obs = self.norm.obs_ring() if self.normalize_obs else mem.obs
        with torch.no_grad():
            self.values = self.value(ring_obs).squeeze(-1).contiguous()
        out = self.advantages.compute(self.values, steps, rewards=self.norm.rewards() if self.normalize_reward else None)
        slots = self.advantages.window(steps)
        take = lambda t: t[slots][:, :, :nl]
        obs = take(ring_obs).reshape(-1, mem.obs.shape[-1])
        u = take(self.u).reshape(-1, 2)
        logp_old = take(self.logp).reshape(-1)
        adv = take(out.adv_norm).reshape(-1)
        ret = take(out.ret).reshape(-1)
        self.weight = weight = ((take(out.valid) != 0) & ~self._parked(slots, mem.count - steps)).reshape(-1).to(torch.float32)
        rows = obs.shape[0]
        size = rows // self.minibatches
        log = {}
        for epoch in range(self.epochs):
            perm = torch.randperm(rows, generator=self.generator, device=self.device)
            log = {"policy_loss": [], "value_loss": [], "entropy": []}
            for j in range(self.minibatches):
                idx = perm[j * size:(j + 1) * size]
                if self.fused_heads:
                    x = obs[idx]
                    mean, log_std = self.policy(x)
                    v = self.value(x).squeeze(-1)
                    with torch.no_grad():
                        out = self.heads.loss(mean.detach(), log_std.detach(), v.detach(), idx, u, logp_old, adv, ret, weight,
                                              self.clip, self.vf_coef, self.ent_coef)
                    self.optimizer.zero_grad(set_to_none=True)
                    torch.autograd.backward([mean, log_std, v], [out.g_mean, out.g_log_std, out.g_v])
                    if self.max_grad_norm is not None:
                        torch.nn.utils.clip_grad_norm_(self.params, self.max_grad_norm)
                    self.optimizer.step()
                    if epoch == 0 and j == 0:
                        self.first_ratio = out.ratio.clone()
                    if epoch == self.epochs - 1:          # out's views are overwritten by the next minibatch
                        log["policy_loss"].append(out.policy_loss.clone())
                        log["value_loss"].append(out.value_loss.clone())
                        log["entropy"].append(out.entropy.clone())
                    continue
                w = weight[idx]
                denom = w.sum().clamp(min=1.0)
                mean, log_std = self.policy(obs[idx])
                logp = log_prob(mean, log_std, u[idx])
                ratio = torch.exp(logp - logp_old[idx])
                if epoch == 0 and j == 0:
                    self.first_ratio = ratio.detach()
                a = adv[idx]
                surrogate = torch.minimum(ratio * a, ratio.clamp(1.0 - self.clip, 1.0 + self.clip) * a)
                policy_loss = -(w * surrogate).sum() / denom
                v = self.value(obs[idx]).squeeze(-1)
                value_loss = (w * (0.5 * (v - ret[idx]) ** 2)).sum() / denom
                entropy = -(w * logp).sum() / denom          # the sample estimate: the squashed Gaussian has no closed form
                loss = policy_loss + self.vf_coef * value_loss - self.ent_coef * entropy
                self.optimizer.zero_grad(set_to_none=True)
                loss.backward()
                if self.max_grad_norm is not None:
                    torch.nn.utils.clip_grad_norm_(self.params, self.max_grad_norm)
                self.optimizer.step()
                log["policy_loss"].append(policy_loss.detach())
                log["value_loss"].append(value_loss.detach())
                log["entropy"].append(entropy.detach())
        if self.normalize_obs:
            self.norm.fold_obs()          # after the last minibatch: the record was frozen while the rollout was evaluated
        self.updates += 1
        return {k: torch.stack(v).mean() for k, v in log.items()}

    # -- snapshot / restore (checkpoint.py) ---------------------------------------------------------------------
    def state_dict(self, include_sampler=True):
        """Tensors and built-in types only: the two networks, Adam's state, the per-slot u and log π (left out with
        include_sampler=False, as the ring then is), the update count; with normalize_obs or normalize_reward also "norm",
        the normalizer's record, carry and counters."""
        sd = {"kind": "ppo", "policy": dict(self.policy.state_dict()), "value": dict(self.value.state_dict()),
              "optimizer": self.optimizer.state_dict(), "updates": int(self.updates)}
        if include_sampler:
            sd["u"], sd["logp"] = self.u, self.logp
        if self.norm is not None:
            sd["norm"] = self.norm.state_dict()
        return sd

    def load_state_dict(self, sd):
        """Restores a state_dict() of a PPO of the same shapes, in place."""
        if not isinstance(sd, dict) or sd.get("kind") != "ppo":
            raise ValueError("uavx: PPO.load_state_dict was given the state of another learner")
        for name in ("u", "logp"):
            if name in sd and (not torch.is_tensor(sd[name]) or tuple(sd[name].shape) != tuple(getattr(self, name).shape)
                               or sd[name].dtype != torch.float32):
                raise ValueError(f"uavx: the saved PPO's {name!r} does not fit this ring")
        if ("norm" in sd) != (self.norm is not None):
            raise ValueError("uavx: the saved PPO was trained %s normalisation, this one is built %s it"
                             % (("with", "without") if "norm" in sd else ("without", "with")))
        if self.norm is not None:
            self.norm.check_state(sd["norm"])
        self.policy.load_state_dict(sd["policy"])
        self.value.load_state_dict(sd["value"])
        self.optimizer.load_state_dict(sd["optimizer"])
        for name in ("u", "logp"):
            if name in sd:
                getattr(self, name).copy_(sd[name])
        if self.norm is not None:
            self.norm.load_state_dict(sd["norm"])
        self.updates = int(sd["updates"])
        return self

    def close(self):
        pass
