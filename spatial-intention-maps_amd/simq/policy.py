"""simq.DQNPolicy -- drop-in for the reference ``policies.DQNPolicy`` (policies.py:11-74).

Same constructor, attributes and methods; each policy net is a simq.FCN (HIP) instead of
DataParallel(networks.FCN).  The three VectorEnv statics the reference calls are replaced by the
constants they return (simq.arch, citing envs.py:366-376,810,1090,2010) because the simulator is
out of scope.  `build_network` / `apply_transition` -- the names BASELINE.json uses -- are aliases
of the reference's real `build_policy_nets` / `apply_transform`.
"""
import random

import numpy as np
import torch

from . import arch
from ._lib import SimqError, lib, ptr, stream_ptr
from .fcn import FCN, is_handle, states_as, states_batch


class DQNPolicy:
    def __init__(self, cfg, train=False, random_seed=None):
        self.cfg = cfg
        self.robot_group_types = [next(iter(g.keys())) for g in self.cfg.robot_config]     # policies.py:14
        self.train = train
        if random_seed is not None:
            random.seed(random_seed)                                                        # policies.py:16-17
        self.num_robot_groups = len(self.robot_group_types)
        if not torch.cuda.is_available():
            raise SimqError('simq.DQNPolicy needs an MI355X (torch.cuda.is_available() is False); no CPU path')
        self.device = torch.device('cuda')                                                  # policies.py:21
        self.policy_nets = self.build_policy_nets()
        # Resume if applicable (policies.py:25-33)
        if getattr(self.cfg, 'checkpoint_path', None) is not None:
            self.policy_checkpoint = torch.load(self.cfg.policy_path, map_location=self.device)
            for i in range(self.num_robot_groups):
                self.policy_nets[i].load_state_dict(self.policy_checkpoint['state_dicts'][i])
                if self.train:
                    self.policy_nets[i].train()
                else:
                    self.policy_nets[i].eval()
            print("=> loaded policy '{}'".format(self.cfg.policy_path))

    def build_policy_nets(self):                                                            # policies.py:35-42
        policy_nets = []
        for robot_type in self.robot_group_types:
            num_output_channels = arch.get_num_output_channels(robot_type)
            policy_nets.append(FCN(num_input_channels=self.cfg.num_input_channels,
                                   num_output_channels=num_output_channels, device=self.device,
                                   precision=getattr(self.cfg, 'simq_precision', 'fp32'),
                                   # simq_plan_options overrides of the Q-networks, e.g. {'bf16_states': 1} for a run on bf16 replay pools:
                                   # such nets step on handles of a bf16 pool as they are and round anything fp32 on the device
                                   options=getattr(self.cfg, 'simq_plan_options', None)))
        return policy_nets

    build_network = build_policy_nets      # BASELINE.json's name for the same call

    def apply_transform(self, s):                                                           # policies.py:44-45
        """ToTensor on a float32 HWC ndarray (no scaling) + unsqueeze(0): [1,C,96,96]."""
        return torch.from_numpy(np.ascontiguousarray(s).transpose(2, 0, 1)).unsqueeze(0)

    apply_transition = apply_transform     # BASELINE.json's name for the same call

    def step(self, state, exploration_eps=None, debug=False):                               # policies.py:47-74
        if exploration_eps is None:
            exploration_eps = self.cfg.final_exploration
        action = [[None for _ in g] for g in state]
        output = [[None for _ in g] for g in state]
        with torch.no_grad():
            for i, g in enumerate(state):
                robot_type = self.robot_group_types[i]
                net = self.policy_nets[i]
                net.eval()
                # the reference runs one batch-1 forward per robot (HWC -> CHW -> device -> net -> argmax -> .cpu()); here
                # all robots of the group share ONE eval forward (eval-mode BatchNorm: samples are independent) and one
                # argmax launch; only the indices come back, the Q-maps only when `debug` asks for them.  The RNG draws
                # stay in the reference's (i, j) order.
                live = [j for j, s in enumerate(g) if s is not None]
                greedy, qmaps = net.infer_argmax_batch([g[j] for j in live], need_q=debug) if live else ([], [])
                for k, j in enumerate(live):
                    if random.random() < exploration_eps:
                        a = random.randrange(arch.get_action_space(robot_type))
                    else:
                        a = greedy[k]
                    action[i][j] = a
                    output[i][j] = qmaps[k] if debug else None
                if self.train:
                    net.train()
        if debug:
            info = {'output': output}
            return action, info
        return action


    def step_many(self, states, exploration_eps=None):
        """`step` for several environments at once (train_multiprocess.py:254-264 serves its collector workers
        one B=1 `policy.step` at a time): the awaiting robots of ALL environments share one eval forward + one argmax launch per
        robot group.  The epsilon-greedy draws are made in the order sequential `step(states[0])`, `step(states[1])`, ... calls
        would make them, so a seeded run selects the same actions.  Returns one action structure per environment."""
        if exploration_eps is None:
            exploration_eps = self.cfg.final_exploration
        actions = [[[None for _ in g] for g in st] for st in states]
        greedy = {}
        with torch.no_grad():
            for i in range(self.num_robot_groups):
                live = [(e, j) for e, st in enumerate(states) for j, s in enumerate(st[i]) if s is not None]
                if not live:
                    continue
                net = self.policy_nets[i]
                net.eval()
                idx, _ = net.infer_argmax_batch([states[e][i][j] for e, j in live], need_q=False)
                for (e, j), a in zip(live, idx):
                    greedy[(e, i, j)] = a
                if self.train:
                    net.train()
        for e, st in enumerate(states):                          # RNG draws: environment by environment, then (i, j) as in step()
            for i, g in enumerate(st):
                for j, s in enumerate(g):
                    if s is None:
                        continue
                    if random.random() < exploration_eps:
                        actions[e][i][j] = random.randrange(arch.get_action_space(self.robot_group_types[i]))
                    else:
                        actions[e][i][j] = greedy[(e, i, j)]
        return actions


class DQNIntentionPolicy(DQNPolicy):
    """Drop-in for policies.DQNIntentionPolicy (policies.py:76-146): one intention net FCN(C-1, 1) per robot group
    predicts the other robots' intention map, which is appended to the state before the Q-network runs.  The predicted
    map never leaves HBM between the two nets unless `debug` asks for it."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.intention_nets = self.build_intention_nets()
        if getattr(self.cfg, 'checkpoint_path', None) is not None:                          # policies.py:80-87
            for i in range(self.num_robot_groups):
                self.intention_nets[i].load_state_dict(self.policy_checkpoint['state_dicts_intention'][i])
                if self.train:
                    self.intention_nets[i].train()
                else:
                    self.intention_nets[i].eval()
            print("=> loaded intention network '{}'".format(self.cfg.policy_path))

    def build_intention_nets(self):                                                         # policies.py:89-95
        # cfg.simq_intention_plan_options: simq_plan_options overrides of the intention nets ({'bf16_states': 1} on bf16 replay pools);
        # cfg.simq_intention_fused: simq.train_intention runs their supervision step as one library call (simq_train_intention_step)
        nets = [FCN(num_input_channels=self.cfg.num_input_channels - 1, num_output_channels=1, device=self.device,
                    precision=getattr(self.cfg, 'simq_precision', 'fp32'),
                    options=getattr(self.cfg, 'simq_intention_plan_options', None)) for _ in range(self.num_robot_groups)]
        for net in nets:
            net.fused_step = bool(getattr(self.cfg, 'simq_intention_fused', False))
        return nets

    def _typed(self, i, states):
        """Whether group i's states take the typed path: some state is bf16 (a handle of a bf16 pool, a bfloat16 tensor), or the
        intention net or the Q-network reads bf16 states.  Then nothing is widened to fp32 on the way: the batch is gathered in the pool's
        type, loses its ground-truth channel in one simq_intention_split into the intention net's type, and one simq_sigmoid_concat_x
        writes state + predicted map in the Q-network's type.  fp32 states and fp32 nets: the calls this class always made."""
        bf = torch.bfloat16
        return (self.intention_nets[i].state_dtype == bf or self.policy_nets[i].state_dtype == bf
                or any((is_handle(s) and s.pool.dtype == bf) or (torch.is_tensor(s) and s.dtype == bf) for s in states))

    def _typed_input(self, i, xs, drop_last):
        """Typed path: the states xs as one batch [n,96,96,C or C-1] in the intention net's type (drop_last: without the ground-truth map)."""
        net = self.intention_nets[i]
        x = xs[0] if len(xs) == 1 and torch.is_tensor(xs[0]) else states_batch(xs, self.device)
        if not drop_last:
            return states_as(x.contiguous(), net.state_dtype)
        n, W, C = x.shape[0], arch.STATE_WIDTH, x.shape[3]
        head = torch.empty((n, W, W, C - 1), dtype=net.state_dtype, device=self.device)
        lib.call('simq_intention_split', ptr(x.contiguous()), int(x.dtype == torch.bfloat16), ptr(head), int(head.dtype == torch.bfloat16), None,
                 n * W * W, C, stream_ptr(self.device))
        return head

    def _concat(self, i, x, logit, prob=None):
        """Typed path: concat(x, sigmoid(logit)) in the Q-network's type."""
        n, W, C = x.shape[0], arch.STATE_WIDTH, x.shape[3]
        out = torch.empty((n, W, W, C + 1), dtype=self.policy_nets[i].state_dtype, device=self.device)
        lib.call('simq_sigmoid_concat_x', ptr(x), int(x.dtype == torch.bfloat16), ptr(logit), ptr(out), int(out.dtype == torch.bfloat16), ptr(prob),
                 n * W * W, C, stream_ptr(self.device))
        return out

    def _predict(self, i, s):
        """One HWC state [96,96,C-1] (ndarray, replay pool handle, or a device tensor [1,96,96,C-1]) -> device tensors
        (state_with_intention [1,96,96,C], sigmoid map [96,96])."""
        net = self.intention_nets[i]
        if self._typed(i, [s]):
            x = self._typed_input(i, [s], False)
            prob = torch.empty((arch.STATE_WIDTH, arch.STATE_WIDTH), dtype=torch.float32, device=self.device)
            return self._concat(i, x, net.forward_nhwc(x), prob), prob
        # (fp32 arithmetic on the state itself -- sigmoid_concat)
        x = s if torch.is_tensor(s) else states_batch([s], self.device, torch.float32) if is_handle(s) else \
            torch.from_numpy(np.ascontiguousarray(s, dtype=np.float32)).unsqueeze(0).to(self.device)
        logit = net.forward_nhwc(x)
        C = x.shape[3]
        out = torch.empty((1, arch.STATE_WIDTH, arch.STATE_WIDTH, C + 1), dtype=torch.float32, device=self.device)
        prob = torch.empty((arch.STATE_WIDTH, arch.STATE_WIDTH), dtype=torch.float32, device=self.device)
        lib.call('simq_sigmoid_concat', ptr(x), ptr(logit), ptr(out), ptr(prob), arch.STATE_WIDTH * arch.STATE_WIDTH, C,
                 stream_ptr(self.device))
        return out, prob

    def step_intention(self, state, debug=False, _device=False):                            # policies.py:97-117
        state_intention = [[None for _ in g] for g in state]
        output_intention = [[None for _ in g] for g in state]
        with torch.no_grad():
            for i, g in enumerate(state):
                self.intention_nets[i].eval()
                for j, s in enumerate(g):
                    if s is not None:
                        out, prob = self._predict(i, s)
                        # (a bf16 state + map of the typed path leaves the device widened exactly: the reference's float32 array)
                        state_intention[i][j] = out if _device else out[0].float().cpu().numpy()
                        if debug:
                            output_intention[i][j] = prob.cpu().numpy()
                if self.train:
                    self.intention_nets[i].train()
        if debug:
            return state_intention, {'output_intention': output_intention}
        return state_intention

    def step(self, state, exploration_eps=None, debug=False, use_ground_truth_intention=False):   # policies.py:119-146
        if self.train and use_ground_truth_intention:
            return super().step(state, exploration_eps=exploration_eps, debug=debug)
        if self.train:                                                                      # drop the ground-truth map
            # (a pool handle is read on the device and loses its last channel there; an ndarray on the host, as always.  Typed path: one
            # simq_intention_split per state, from the pool's type into the intention net's)
            typed = [self._typed(i, [s for s in g if s is not None]) for i, g in enumerate(state)]
            state = [[None if s is None else self._typed_input(i, [s], True) if typed[i] else
                      states_batch([s], self.device, torch.float32)[..., :-1].contiguous() if is_handle(s) else s[:, :, :-1]
                      for s in g] for i, g in enumerate(state)]
        state = self.step_intention(state, debug=debug, _device=not debug)
        if debug:
            state, info_intention = state
        action = super().step(state, exploration_eps=exploration_eps, debug=debug)
        if debug:
            action, info = action
            info['state_intention'] = state
            info['output_intention'] = info_intention['output_intention']
            return action, info
        return action

    def step_many(self, states, exploration_eps=None, use_ground_truth_intention=False):
        """Several environments at once, predicted-intention path included: per robot group ONE batched forward of
        the intention net over the awaiting robots of all environments, one sigmoid+concat launch over the whole batch (the predicted
        maps stay in HBM), then the batched Q-network forward + argmax of DQNPolicy.step_many.  Same results and the same
        epsilon-greedy draw order as sequential step() calls (policies.py:119-146)."""
        if self.train and use_ground_truth_intention:
            return super().step_many(states, exploration_eps=exploration_eps)
        W = arch.STATE_WIDTH
        pred = [[[None for _ in g] for g in st] for st in states]
        with torch.no_grad():
            for i in range(self.num_robot_groups):
                live = [(e, j) for e, st in enumerate(states) for j, s in enumerate(st[i]) if s is not None]
                if not live:
                    continue
                net = self.intention_nets[i]
                net.eval()                                                                 # policies.py:101
                xs = [states[e][i][j] for e, j in live]
                if self._typed(i, xs):                                                     # nothing widened: see _typed
                    x = self._typed_input(i, xs, self.train)
                    out = self._concat(i, x, net.forward_nhwc(x))
                    for k, (e, j) in enumerate(live):
                        pred[e][i][j] = out[k:k + 1]
                    if self.train:
                        net.train()
                    continue
                if any(is_handle(s) for s in xs):                                          # pool handles: the batch is formed in HBM
                    x = states_batch(xs, self.device, torch.float32)   # (handles of a bf16 pool: widened exactly, as in _predict)
                    if self.train:
                        x = x[..., :-1].contiguous()
                else:
                    if self.train:                                                         # drop the ground-truth map (policies.py:124)
                        xs = [s[:, :, :-1] for s in xs]
                    x = torch.from_numpy(np.stack([np.ascontiguousarray(s, dtype=np.float32) for s in xs])).to(self.device)
                logit = net.forward_nhwc(x)
                n, C = x.shape[0], x.shape[3]
                out = torch.empty((n, W, W, C + 1), dtype=torch.float32, device=self.device)
                lib.call('simq_sigmoid_concat', ptr(x), ptr(logit), ptr(out), None, n * W * W, C, stream_ptr(self.device))
                for k, (e, j) in enumerate(live):
                    pred[e][i][j] = out[k:k + 1]
                if self.train:
                    net.train()
        return super().step_many(pred, exploration_eps=exploration_eps)
