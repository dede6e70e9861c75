"""Host-side checks of the learner bindings' shared layer: _actor_lib's table of units gives the
sources and every public constant the hand-written module gave (values recorded at commit 1ba5a5c; the tenth unit, the
n-step sampler, and the per-file hashes at 9a32f7c; the eleventh unit, the weighted critic gradient, at the commit that
folded it into uavx_critic_grad.hip), covers every exported symbol, and every class built on the kind
tables and on critic_handle refuses a wrong class, a wrong pair and a CPU module with the message it had there -- before
the library is loaded, so without a GPU."""
import hashlib
import json
import os
import re

import pytest
import torch

from gym_uav_collision_avoidance_amd import _actor_lib, _native, policy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# source_hash() at the commit that folded the weighted critic gradient into uavx_critic_grad.hip, the second commit that moved
# it on purpose (a056e385b4f6651e before it, from the commit that moved the n-step sampler into uavx_replay.hip;
# ab517ee91bb05350 before that), and moved once more, from 17c0e2c29cadcdb4, when uavx_replay.hip took the replay ring's view,
# the n-step walk and the entry plumbing from common_csrc/
MERGED_HASH = "c6725b15f59f1983"
PARENT_SOURCES = [
    "uavx_action_grad.hip", "uavx_actor.hip", "uavx_actor_impl.hpp", "uavx_critic.hip", "uavx_critic_grad.hip",
    "uavx_explore.hip", "uavx_grad_common.hip", "uavx_grad_impl.hpp", "uavx_learner.hip", "uavx_optim.hip",
    "uavx_policy_grad.hip", "uavx_replay.hip", "uavx_actor.h", "uavx_critic.h", "uavx_critic_grad.h", "uavx_optim.h",
    "uavx_replay.h", "uavx_action_grad.h", "uavx_policy_grad.h", "uavx_learner.h", "uavx_explore.h", "uavx_nstep.h",
    "uavx_wcritic_grad.h", "uavx_entry.hpp", "uavx_replay_ring.hpp", "uavx_replay_walk.hpp"]
UNIT_NAMES = ("", "CRITIC_", "GRAD_", "OPTIM_", "REPLAY_", "ACTION_GRAD_", "POLICY_GRAD_", "LEARNER_", "EXPLORE_",
              "NSTEP_", "WGRAD_")
PARENT_HEADERS = ("uavx_actor.h", "uavx_critic.h", "uavx_critic_grad.h", "uavx_optim.h", "uavx_replay.h",
                  "uavx_action_grad.h", "uavx_policy_grad.h", "uavx_learner.h", "uavx_explore.h", "uavx_nstep.h",
                  "uavx_wcritic_grad.h")
PARENT_SYMBOLS = (
    ("uavx_actor_version", "uavx_actor_strerror", "uavx_actor_create", "uavx_actor_destroy", "uavx_actor_pack",
     "uavx_actor_forward"),
    ("uavx_critic_version", "uavx_critic_strerror", "uavx_critic_create", "uavx_critic_destroy",
     "uavx_critic_set_split_rows", "uavx_critic_pack", "uavx_critic_q", "uavx_critic_target"),
    ("uavx_critic_grad_version", "uavx_critic_grad_workspace_bytes", "uavx_critic_grad"),
    ("uavx_optim_version", "uavx_optim_adam", "uavx_optim_soft_update"),
    ("uavx_replay_version", "uavx_replay_workspace_bytes", "uavx_replay_sample"),
    ("uavx_action_grad_version", "uavx_action_grad"),
    ("uavx_policy_grad_version", "uavx_policy_grad_workspace_bytes", "uavx_policy_grad_forward",
     "uavx_policy_grad_backward"),
    ("uavx_learner_version", "uavx_learner_tail"),
    ("uavx_explore_version", "uavx_explore_act"),
    ("uavx_nstep_version", "uavx_nstep_workspace_bytes", "uavx_nstep_sample"),
    ("uavx_wcritic_grad_version", "uavx_wcritic_grad_workspace_bytes", "uavx_wcritic_grad"))
PARENT_CONSTANTS = dict(
    SAC=0, TD3=1, DDPG=2, F32=0, BF16=1, RAW=0, DETERMINISTIC=1, SAC_SAMPLE=2, ADD_CLAMP=3, OK=0, ERR_INVALID_ARG=-1,
    ERR_HIP=-2, ERR_UNSUPPORTED=-3, ERR_NOT_PACKED=-4, SPLIT_ROWS=16384, GRAD_MSE=0, GRAD_L1=1, GRAD_MAX_ROWS=262144,
    OPTIM_MAX_TENSORS=16, REPLAY_MAX_ROWS=1048576, REPLAY_SINGLE_ROWS=1024, ACTION_GRAD_MAX_ROWS=262144,
    POLICY_GRAD_MAX_ROWS=262144, LEARNER_LOG_COLUMNS=8, EXPLORE_MAX_ROWS=16777216, EXPLORE_STATE_BYTES=16, NSTEP_MAX=8,
    NSTEP_MAX_ROWS=1048576, NSTEP_SINGLE_ROWS=1024)
WORDS = ("actor", "critic", "critic-gradient", "optimiser", "replay", "action-gradient", "policy-gradient", "learner",
         "exploration", "n-step replay", "weighted critic-gradient")


def test_hash_and_sources_are_the_parents():
    """Nothing outside the replay unit and the critic-gradient unit moved: every source but uavx_replay.hip and
    uavx_critic_grad.hip has the code it had at 9a32f7c (golden/actor_sources_parent.json, written there by
    golden/make_actor_sources.py), and the only files the library gained are the n-step header and the weighted
    critic gradient's, and the three headers of common_csrc/ that uavx_replay.hip includes.  The hash moved three times, each
    time for one unit: when the n-step sampler joined uavx_replay.hip, when the weighted critic gradient, until then a
    restatement of grad_rows in a library of its own, became a template switch of grad_rows, and when what
    the replay unit had alike with the prio and keywalk libraries went to common_csrc/ (§21)."""
    sources = _actor_lib._sources()
    assert [os.path.basename(p) for p in sources] == PARENT_SOURCES
    assert all(os.path.isfile(p) for p in sources)
    parent = json.load(open(os.path.join(ROOT, "tests", "golden", "actor_sources_parent.json")))
    gained = {"uavx_nstep.h", "uavx_wcritic_grad.h", "uavx_entry.hpp", "uavx_replay_ring.hpp", "uavx_replay_walk.hpp"}
    assert set(PARENT_SOURCES) == set(parent) | gained and not gained & set(parent)
    for p in sources:
        name = os.path.basename(p)
        if name not in ("uavx_replay.hip", "uavx_critic_grad.hip") and name not in gained:
            code = _native.code_only(open(p, encoding="utf-8").read())
            assert hashlib.sha256(code.encode()).hexdigest() == parent[name], name
    assert _actor_lib.source_hash() == MERGED_HASH


def test_public_constants_keep_their_parent_values():
    for name, value in PARENT_CONSTANTS.items():
        assert getattr(_actor_lib, name) == value, name
    pkg = os.path.join(ROOT, "gym_uav_collision_avoidance_amd")
    assert _actor_lib.CSRC == os.path.join(pkg, "actor_csrc")
    assert _actor_lib.LIB_PATH == os.path.join(pkg, "actor_csrc", "libuavx_actor.so")
    for prefix, header, symbols in zip(UNIT_NAMES, PARENT_HEADERS, PARENT_SYMBOLS):
        assert getattr(_actor_lib, prefix + "HEADER") == os.path.join(ROOT, "include", header), prefix
        assert getattr(_actor_lib, prefix + "SYMBOLS") == symbols, prefix
        assert getattr(_actor_lib, prefix + "ABI_VERSION") == 1, prefix
    ring = [n for n, _ in _actor_lib.ReplayRing._fields_]
    assert ring == ["obs", "act", "rew", "done", "skip", "trunc", "ended", "slots", "envs", "agents", "learners"]
    assert len(_actor_lib.ExploreArgs._fields_) == 25 and _actor_lib.ExploreArgs._fields_[0][0] == "kind"


def test_the_table_covers_every_symbol_and_load_binds_it():
    units = _actor_lib.UNITS
    assert tuple(u.word for u in units) == WORDS
    for u, symbols in zip(units, PARENT_SYMBOLS):
        assert tuple(u.functions) == symbols and u.version == symbols[0] and u.version.endswith("_version")
        declared = set(re.findall(r"\b(uavx_[a-z_0-9]+)\s*\(", open(u.header).read()))
        assert set(symbols) <= declared, set(symbols) - declared
    _actor_lib.build()
    lib = _actor_lib.load()
    for u in units:
        for name, (restype, argtypes) in u.functions.items():
            f = getattr(lib, name)
            assert f.restype is restype and list(f.argtypes) == list(argtypes), name
    assert lib.uavx_actor_strerror(_actor_lib.ERR_INVALID_ARG) == b"invalid argument"


def _refusals():
    from gym_uav_collision_avoidance_amd.fused_actor import FusedActor
    from gym_uav_collision_avoidance_amd.fused_critic import (FusedActionGrad, FusedActorLoss, FusedCritic,
                                                              FusedCriticLoss, FusedTarget)
    from gym_uav_collision_avoidance_amd.fused_policy_grad import FusedPolicyGrad
    p = policy
    lin = torch.nn.Linear(12, 1)
    gpu = " needs the module on a GPU (cuda:N), its parameters are on cpu"
    critic_or_handle = " takes a TwinQ, TD3TwinQ, DDPGCritic or FusedCritic, not "
    precision = "uavx: precision must be one of ['bf16', 'f32'], not 'f16'"
    bad_loss = "uavx: loss must be one of ['l1', 'mse'] or None, not 'huber'"
    return [
        (lambda: FusedActor(lin), TypeError, "uavx: FusedActor takes a GaussianPolicy, TD3Actor or DDPGActor, not Linear"),
        (lambda: FusedActor(p.TwinQ()), TypeError, "uavx: FusedActor takes a GaussianPolicy, TD3Actor or DDPGActor, not TwinQ"),
        (lambda: FusedActor(p.TD3Actor(), precision="f16"), ValueError, precision),
        (lambda: FusedActor.from_module(p.GaussianPolicy()), ValueError, "uavx: FusedActor" + gpu),
        (lambda: FusedActor(p.DDPGActor()), ValueError, "uavx: FusedActor" + gpu),
        (lambda: FusedCritic(lin), TypeError, "uavx: FusedCritic takes a TwinQ, TD3TwinQ or DDPGCritic, not Linear"),
        (lambda: FusedCritic(p.TD3Actor()), TypeError, "uavx: FusedCritic takes a TwinQ, TD3TwinQ or DDPGCritic, not TD3Actor"),
        (lambda: FusedCritic(p.TwinQ(), precision="f16"), ValueError, precision),
        (lambda: FusedCritic.from_module(p.TD3TwinQ()), ValueError, "uavx: FusedCritic" + gpu),
        (lambda: FusedCritic(p.DDPGCritic()), ValueError, "uavx: FusedCritic" + gpu),
        (lambda: FusedTarget(lin, p.TwinQ()), TypeError, "uavx: FusedActor takes a GaussianPolicy, TD3Actor or DDPGActor, not Linear"),
        (lambda: FusedTarget(p.TD3Actor(), p.TD3TwinQ()), ValueError, "uavx: FusedActor" + gpu),
        (lambda: FusedTarget(p.GaussianPolicy(), p.TwinQ(), precision="f16"), ValueError, precision),
        (lambda: FusedCriticLoss(p.TD3Actor()), TypeError, "uavx: FusedCriticLoss" + critic_or_handle + "TD3Actor"),
        (lambda: FusedCriticLoss(lin, loss="huber"), TypeError, "uavx: FusedCriticLoss" + critic_or_handle + "Linear"),
        (lambda: FusedCriticLoss(p.TwinQ(), loss="huber"), ValueError, bad_loss),
        (lambda: FusedCriticLoss(p.TwinQ()), ValueError, "uavx: FusedCriticLoss" + gpu),
        (lambda: FusedCriticLoss(p.DDPGCritic(), loss="l1"), ValueError, "uavx: FusedCriticLoss" + gpu),
        (lambda: FusedActionGrad(p.TD3Actor()), TypeError, "uavx: FusedActionGrad" + critic_or_handle + "TD3Actor"),
        (lambda: FusedActionGrad(lin), TypeError, "uavx: FusedActionGrad" + critic_or_handle + "Linear"),
        (lambda: FusedActionGrad(p.TD3TwinQ()), ValueError, "uavx: FusedActionGrad" + gpu),
        (lambda: FusedActorLoss(p.TwinQ(), p.TwinQ()), TypeError,
         "uavx: FusedActorLoss takes a GaussianPolicy, TD3Actor or DDPGActor, not TwinQ"),
        (lambda: FusedActorLoss(p.TD3Actor(), lin), TypeError, "uavx: FusedActionGrad" + critic_or_handle + "Linear"),
        (lambda: FusedActorLoss(p.TD3Actor(), p.TD3TwinQ()), ValueError, "uavx: FusedActionGrad" + gpu),
        (lambda: FusedPolicyGrad(p.TwinQ(), p.TwinQ()), TypeError,
         "uavx: FusedPolicyGrad takes a GaussianPolicy, TD3Actor or DDPGActor, not TwinQ"),
        (lambda: FusedPolicyGrad(p.TD3Actor(), p.TD3Actor()), TypeError,
         "uavx: FusedPolicyGrad takes a TwinQ, TD3TwinQ, DDPGCritic, FusedCritic or FusedActionGrad as its critic, not "
         "TD3Actor"),
        (lambda: FusedPolicyGrad(p.TD3Actor(), p.TwinQ()), TypeError,
         "uavx: FusedPolicyGrad pairs a TD3 actor (TD3Actor) with a SAC critic (TwinQ)"),
        (lambda: FusedPolicyGrad(p.GaussianPolicy(), p.DDPGCritic()), TypeError,
         "uavx: FusedPolicyGrad pairs a SAC actor (GaussianPolicy) with a DDPG critic (DDPGCritic)"),
        (lambda: FusedPolicyGrad(p.DDPGActor(), p.DDPGCritic()), ValueError,
         "uavx: FusedPolicyGrad needs the actor on a GPU (cuda:N), its parameters are on cpu"),
    ]


def test_every_class_refuses_bad_modules_before_the_device_with_the_parents_text():
    for call, cls, message in _refusals():
        with pytest.raises(cls, match="^" + re.escape(message) + "$"):
            call()


def test_kind_tables_name_the_layers_in_the_kernels_order():
    from gym_uav_collision_avoidance_amd._fused_common import actor_layers, critic_layers
    sac, td3, ddpg = policy.GaussianPolicy(), policy.TD3Actor(), policy.DDPGActor()
    assert actor_layers(sac) == (_actor_lib.SAC, (sac.linear1, sac.linear2, sac.mean_linear, sac.log_std_linear))
    assert actor_layers(td3) == (_actor_lib.TD3, (td3.l1, td3.l2, td3.l3))
    assert actor_layers(ddpg) == (_actor_lib.DDPG, (ddpg.input, ddpg.fc1, ddpg.fc2))
    tw, tq, dc = policy.TwinQ(), policy.TD3TwinQ(), policy.DDPGCritic()
    assert critic_layers(tw) == (_actor_lib.SAC, (tw.linear1, tw.linear2, tw.linear3, tw.linear4, tw.linear5, tw.linear6))
    assert critic_layers(tq) == (_actor_lib.TD3, (tq.l1, tq.l2, tq.l3, tq.l4, tq.l5, tq.l6))
    assert critic_layers(dc) == (_actor_lib.DDPG, (dc.input, dc.fc1, dc.fc2))
    assert actor_layers(tw) is None and critic_layers(sac) is None and actor_layers(torch.nn.Linear(2, 2)) is None
