"""Names, shapes and copies of the networks' flat parameter vectors: the
actor's and the critic's flat layouts (include/lnw.h; PPOLearner's theta_actor
and theta_critic, Rollout's `theta`), the Q-net's packed() layout (lnw_qnet_act,
QLearner's theta), and the copy of a module's parameters and running statistics
into such a vector and back. No network code: the forward passes that read
these layouts are lnw/nets.py's.
"""
import numpy as np
import torch

WINDOW = 49  # the 7x7 terrain window at the head of a Combatant observation
CONV_PARAMS = 578  # the conv head's packed floats (csrc/lnw_convhead.inc)
N_RADAR, N_ATTACK, N_MOVE = 2, 5, 50  # DMLP's heads (network.py:261-263)

# the conv head in lnw_actor_features' order (csrc/lnw_actor.hip): conv1 w, b;
# norm1 w, b, running mean, var; conv2 w, b; norm2 w, b, running mean, var;
# convhead w, b
CONV_HEAD = (("conv1.weight", (5, 1, 3, 3)), ("conv1.bias", (5,)), ("norm1.weight", (5,)), ("norm1.bias", (5,)),
             ("norm1.running_mean", (5,)), ("norm1.running_var", (5,)), ("conv2.weight", (8, 5, 3, 3)),
             ("conv2.bias", (8,)), ("norm2.weight", (8,)), ("norm2.bias", (8,)), ("norm2.running_mean", (8,)),
             ("norm2.running_var", (8,)), ("convhead.weight", (12, 8)), ("convhead.bias", (12,)))
RUNNING = ("norm1.running_mean", "norm1.running_var", "norm2.running_mean", "norm2.running_var")


def _slices(table):
    out, k = {}, 0
    for name, shp in table:
        out[name] = (k, tuple(shp))
        k += int(np.prod(shp))
    return out


def actor_slices(n_in):
    """{state_dict name: (offset, shape)} of the actor's flat layout
    (include/lnw.h): BatchedActor.packed_features()'s order, then fc1 / fc2 / fc3
    weight and bias, normal_head, log_std_head and a slot for logstd."""
    return _slices(CONV_HEAD + (("layernorm.weight", (n_in,)), ("layernorm.bias", (n_in,)),
                                ("fc1.weight", (64, n_in)), ("fc1.bias", (64,)), ("fc2.weight", (64, 64)),
                                ("fc2.bias", (64,)), ("fc3.weight", (32, 64)), ("fc3.bias", (32,)),
                                ("normal_head.weight", (4, 32)), ("log_std_head.weight", (4, 32)), ("logstd", ())))


def critic_slices(n, D):
    """{state_dict name: (offset, shape)} of the critic's flat layout: the
    state_dict order."""
    return _slices((("fc1.weight", (32, n * D)), ("fc1.bias", (32,)), ("fc2.weight", (64, 32)), ("fc2.bias", (64,)),
                    ("fc3.weight", (64, 64)), ("fc3.bias", (64,)), ("fc4.weight", (1, 64)), ("fc4.bias", (1,))))


def packed_slices(n_in):
    """{state_dict name: (offset, shape)} of packed()'s layout for n_in head inputs."""
    return _slices(CONV_HEAD + (("radar.weight", (N_RADAR, n_in)), ("attack.weight", (N_ATTACK, n_in)),
                                ("movement.weight", (N_MOVE, n_in)), ("radar.bias", (N_RADAR,)),
                                ("attack.bias", (N_ATTACK,)), ("movement.bias", (N_MOVE,))))


# the layouts' names in order (state_dict keys); PACKED_NAMES: packed()'s segments
ACTOR_NAMES, CRITIC_NAMES, PACKED_NAMES = tuple(actor_slices(12)), tuple(critic_slices(1, 1)), tuple(packed_slices(12))


def flat_size(sl):
    return max(k + int(np.prod(s)) for k, s in sl.values())


def pack(module, sl):
    """The module's parameters and running statistics as a flat float32 vector."""
    sd = module.state_dict()
    return torch.cat([sd[name].detach().reshape(-1).float() for name in sl]).contiguous()


def unpack_(module, flat, sl):
    """The inverse of pack(): copy a flat vector in the layout sl into the
    module's parameters and running statistics, in place, on the device they
    live on."""
    sd = module.state_dict()  # (tensors sharing the module's storage)
    for name, (k, shp) in sl.items():
        sd[name].copy_(flat[k:k + int(np.prod(shp))].reshape(shp))
    return module


def seg(theta, sl, name):
    """The segment `name` of a flat vector in the layout sl, in its shape (a view)."""
    k, shp = sl[name]
    return theta[k:k + int(np.prod(shp))].reshape(shp)
