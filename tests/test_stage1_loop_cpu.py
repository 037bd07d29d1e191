"""The one step loop of the joint stage-1 trainers (``active_joint_multi.ActiveTrainer.train_impl``) on stub collaborators: every
method runs THAT loop, in the order batch -> zero_grad -> losses -> update -> meters -> logs, with ``flush_meters`` and
``check_stream_k`` once at the end; every method's objective and meter names are what they were when each trainer had a loop of its
own; ``eval_mode`` restores every module's mode; ``args.freeze_bn`` holds for a trainer that used to ignore it.  No GPU, no library
call."""
import importlib
import types

import pytest
import torch
import torch.nn as nn

from mulactseg_amd.models import eval_mode
from mulactseg_amd.trainer import active, active_joint_multi
from mulactseg_amd.utils.scheduler import ramp_up

ARGS = dict(coeff=16.0, coeff_mc=8.0, coeff_gm=0.5, entcoeff=0.25, lamparam=0.1, lamscale=2.0, dorampup=True, simw_temp=0.3,
            simw_temp_schedule=True)
TOTAL = 3
V = (1.25, 2.5, 0.375)          # the stub loss values: distinct, finite, exact in f32


def _ramp(it):
    return ramp_up(it / TOTAL, lamparam=ARGS['lamparam'], scale=ARGS['lamscale'], dorampup=ARGS['dorampup'])


def _pos_group(v, it):
    return ARGS['coeff'] * v[0] + v[1]


def _decomp(v, it):                 # (group, ce, mc)
    return (ARGS['coeff'] * v[1]) + (ARGS['coeff_mc'] * v[2]) + (ARGS['coeff_gm'] * v[0])


def _decomp_no_group(v, it):
    return (ARGS['coeff'] * v[1]) + (ARGS['coeff_mc'] * v[2])


def _online(v, it):                 # (pos, proto)
    return ARGS['coeff'] * v[0] + _ramp(it) * v[1]


# method -> (hook, number of values the hook returns, meters after train-loss with the index of their value, train-loss formula)
POS_GROUP = ('step_losses', 2, (('pos-loss', 0), ('group-loss', 1)), _pos_group)
DECOMP = ('losses', 3, (('ce-loss', 1), ('pos-loss', 2), ('group-loss', 0)), _decomp)
NO_GROUP = ('losses', 3, (('ce-loss', 1), ('pos-loss', 2)), _decomp_no_group)
ONLINE = ('step_losses', 2, (('pos-loss', 0), ('local-proto-loss', 1)), _online)
TABLE = {
    'active_joint_multi': POS_GROUP,
    'active_joint_multi_predignore': POS_GROUP,
    'active_joint_multi_predignore_wgroup': POS_GROUP,
    'active_joint_hier_multi': POS_GROUP,
    'active_joint_hier_multi_async': POS_GROUP,
    'active_joint_hier_multi_async_weight': POS_GROUP,
    'active_joint_multi_predignore_lossdecomp': DECOMP,
    'active_joint_multi_lossdecomp': DECOMP,
    'active_joint_multi_lossdecomp_rc': NO_GROUP,
    'active_joint_multi_lossdecomp_topone': NO_GROUP,
    'active_onlineplbl_multi_predignore': ONLINE,
    'active_onlinewplbl_multi_predignore': ONLINE,
    'active_onlinesimwplbl_multi_predignore': ONLINE,
    'active_onlinewplblonly_multi_predignore': ('step_losses', 2, (), lambda v, it: v[1]),
    'active_pwce_multi_predignore': ('step_loss', 1, (), lambda v, it: v[0]),
    'active_joint_multi_predignore_top1plbl': ('step_losses', 3, (('pos-loss', 0), ('group-loss', 1), ('top1-loss', 2)),
                                               lambda v, it: ARGS['coeff'] * v[0] + v[1] + _ramp(it) * v[2]),
    'active_joint_multi_predignore_multient': ('step_losses', 3, (('pos-loss', 0), ('group-loss', 1), ('ent-loss', 2)),
                                               lambda v, it: ARGS['coeff'] * v[0] + v[1] + ARGS['entcoeff'] * v[2]),
}
SIMW_SCHEDULE_ITERATIONS = 2        # (patched into the pwce module: iterations 0 and 1 run at the schedule's temperature, 2 at the user's)


def _trainer_class(method):
    return importlib.import_module("mulactseg_amd.trainer." + method).ActiveTrainer


class _Net(nn.Module):
    """two parameters and a BatchNorm; ``forward`` accepts ``lowres=``"""

    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(3, 4, 1, bias=False)
        self.bn = nn.BatchNorm2d(4, affine=False)
        self.head = nn.Conv2d(4, 2, 1, bias=False)

    def forward(self, images, lowres=False):
        return self.head(self.bn(self.conv(images)))

    def feat_forward(self, images):
        feats = self.bn(self.conv(images))
        return feats, self.head(feats)


def _batch(cls):
    return tuple(torch.full((1, 3, 4, 4), float(i)) for i in range(len(cls.batch_keys)))


def _stub(method, net=None, **extra_args):
    """(trainer on stub collaborators, the list its calls are recorded in)"""
    cls = _trainer_class(method)
    hook, n_values, _, _ = TABLE[method]
    tr, calls = object.__new__(cls), []
    tr.args = types.SimpleNamespace(**ARGS, **extra_args)
    tr.net, tr.ddp = net if net is not None else _Net(), None
    tr.optimizer = types.SimpleNamespace(zero_grad=lambda: calls.append(('zero_grad',)))
    tr.fused_loss = None
    tr.simw_temp_orig = ARGS['simw_temp']
    tr._batch = lambda: (calls.append(('_batch',)), _batch(cls))[1]

    def losses(*a):
        calls.append((hook, a))
        values = [torch.tensor(v, requires_grad=True) for v in V[:n_values]]
        if method == 'active_onlinewplblonly_multi_predignore':
            values[0] = None
        return values[0] if n_values == 1 else tuple(values)

    setattr(tr, hook, losses)
    tr.update = lambda loss: calls.append(('update', loss))
    tr.update_average_meter = lambda values: calls.append(('update_average_meter', dict(values)))
    tr.log_training = lambda iteration, pbar, total_itrs: calls.append(('log_training', iteration, pbar, total_itrs))
    tr.log_validation = lambda iteration, val_period: calls.append(('log_validation', iteration, val_period))
    tr.flush_meters = lambda: calls.append(('flush_meters',))
    tr.check_stream_k = lambda: calls.append(('check_stream_k',))
    return tr, calls


@pytest.mark.parametrize("method", sorted(TABLE))
def test_every_joint_trainer_runs_the_one_loop(method):
    cls, joint = _trainer_class(method), active_joint_multi.ActiveTrainer
    assert issubclass(cls, joint)
    assert cls.train_impl is joint.train_impl
    assert cls.teacher_forward is joint.teacher_forward and cls.pseudo_label_forward is joint.pseudo_label_forward
    assert active.ActiveTrainer.train_impl is not joint.train_impl      # the plain CE loop stays its own


@pytest.mark.parametrize("method", sorted(TABLE))
def test_call_order_meters_and_objective(method, monkeypatch):
    hook, _, meters, formula = TABLE[method]
    if hook == 'step_loss':
        monkeypatch.setattr(importlib.import_module("mulactseg_amd.trainer." + method), 'SIMW_SCHEDULE_ITERATIONS', SIMW_SCHEDULE_ITERATIONS)
    tr, calls = _stub(method)
    tr.net.eval()
    tr.train_impl(TOTAL, 1000)
    assert tr.net.training and tr.net.bn.training                   # net.train() ran, and nothing froze the BatchNorm (freeze_bn unset)
    per_step = ['_batch', 'zero_grad', hook, 'update', 'update_average_meter', 'log_training', 'log_validation']
    assert [c[0] for c in calls] == per_step * TOTAL + ['flush_meters', 'check_stream_k']
    for it in range(TOTAL):
        _, _, (_, hook_args), (_, loss), (_, values), log_t, log_v = calls[it * len(per_step):(it + 1) * len(per_step)]
        batch = _batch(type(tr))
        n_batch = len(type(tr).batch_keys)
        if hook == 'losses':                            # (logits of forward_train(images), then the rest of the batch)
            assert tuple(hook_args[0].shape) == (1, 2, 4, 4) and hook_args[0].requires_grad
            hook_args, batch = hook_args[1:], batch[1:]
            n_batch -= 1
        assert len(hook_args) >= n_batch and all(torch.equal(x, y) for x, y in zip(hook_args[:n_batch], batch))       # the batch, in its order
        if hook == 'step_loss':
            assert hook_args[n_batch:] == (1000.0 if it < SIMW_SCHEDULE_ITERATIONS else ARGS['simw_temp'],)
        else:
            assert len(hook_args) == n_batch
        assert list(values) == ['train-loss'] + [k for k, _ in meters]
        assert values['train-loss'] is loss and loss.requires_grad
        want = formula([torch.tensor(v) for v in V], it)
        assert loss.item() == want.item(), (it, loss.item(), want.item())
        for key, i in meters:
            assert values[key].item() == V[i]
        assert log_t == ('log_training', it, None, TOTAL) and log_v == ('log_validation', it, 1000)
    if method in ('active_onlineplbl_multi_predignore', 'active_joint_multi_predignore_top1plbl'):
        # the ramp moved between iterations 0 and 2, and is 0 at the start: the schedules saw `iteration` and `total_itrs`
        assert _ramp(0) == 0.0 and 0.0 < _ramp(2) < ARGS['lamscale']
        first, last = calls[3][1], calls[2 * len(per_step) + 3][1]
        assert first.item() != last.item()


def _modes(net):
    return [m.training for m in net.modules()]


@pytest.mark.parametrize("raises", [False, True])
def test_eval_mode_restores_every_module(raises):
    net = nn.Sequential(nn.Conv2d(3, 4, 1), nn.BatchNorm2d(4), nn.Sequential(nn.ReLU(), nn.BatchNorm2d(4)))
    net.train()
    net[1].eval()                                   # one BatchNorm frozen by hand
    before = _modes(net)
    assert before == [True, True, False, True, True, True]
    try:
        with eval_mode(net) as inside:
            assert inside is net and not any(_modes(net)) and not torch.is_grad_enabled()
            if raises:
                raise KeyError("body")
    except KeyError:
        assert raises
    assert _modes(net) == before and torch.is_grad_enabled()


def test_freeze_bn_holds_in_a_trainer_that_ignored_it():
    method = 'active_onlineplbl_multi_predignore'
    net = _Net()
    net.bn = nn.BatchNorm2d(4)                      # affine: freeze_bn also fixes its weight and bias
    tr, calls = _stub(method, net=net, freeze_bn=True)
    seen = []

    def step_losses(images, labels, superpixels, spmasks):
        seen.append((net.training, net.bn.training))
        feats, logits = tr.pseudo_label_forward(images, False)
        seen.append((net.training, net.bn.training))
        assert not logits.requires_grad
        return torch.tensor(V[0], requires_grad=True), torch.tensor(V[1], requires_grad=True)

    tr.step_losses = step_losses
    tr.train_impl(2, 1000)
    assert seen == [(True, False)] * 4              # the root trains, the BatchNorm stays frozen across the eval-mode forward
    net.train()                                     # what log_validation() does after each evaluation
    assert net.training and net.conv.training and not net.bn.training
    assert not net.bn.weight.requires_grad and not net.bn.bias.requires_grad and net.conv.weight.requires_grad
