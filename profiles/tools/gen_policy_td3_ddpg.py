"""Write tests/golden/policy_td3_ddpg.npz: the reference's TD3 / DDPG actor networks evaluated by their own forward().

    python profiles/tools/gen_policy_td3_ddpg.py --reference <checkout of the reference project>

Imports the reference's examples/network.py unchanged (TD3ActorNetwork, DDPGActorNetwork: mean = action_scaling *
tanh(h3(relu(h2(relu(h1(s))))))) and stores, per network and shape, the weights, the inputs, the action_scaling and the
outputs -- data only, nothing of the reference's code.  iiwa (18 -> 5) and planar (12 -> 3) shapes with n_features [64, 64]:
one weight set per shape, evaluated by both classes with action_scaling 1 and with a non-uniform vector.  Keys:
<env>._h{1,2,3}.{weight,bias}, <env>.x, <env>_<unit|vec>.action_scaling, <td3|ddpg>_<env>_<unit|vec>.y.  Like G8 (policy_net.npz), this pins the networks; the noise
processes are restated in tests/policy_explore_oracle.py.
"""
import argparse
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='root of the reference project (holds examples/network.py)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'policy_td3_ddpg.npz'))
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location('ref_network', os.path.join(args.reference, 'examples', 'network.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rng = np.random.default_rng(29)
    out = {}
    for env, n_in, n_out in (('iiwa', 18, 5), ('planar', 12, 3)):
        # one weight set per shape, loaded into both classes (the two actors are the same architecture): keeps the file small
        torch.manual_seed(7 + n_in)
        base = mod.TD3ActorNetwork((n_in,), (n_out,), [64, 64], action_scaling=np.ones(n_out), use_cuda=False)
        with torch.no_grad():
            # the reference initialises h3 in +-3e-3: the tanh would never leave its linear range -- widen it (and the
            # biases) so that the fixture exercises the squash
            base._h3.weight.uniform_(-0.4, 0.4)
            for lin in (base._h1, base._h2, base._h3):
                lin.bias.uniform_(-0.3, 0.3)
        for k, v in base.state_dict().items():
            out[env + '.' + k] = v.numpy()
        x = rng.uniform(-2, 2, (16, n_in)).astype(np.float32)
        out[env + '.x'] = x
        for sc_tag, scaling in (('unit', np.ones(n_out)), ('vec', rng.uniform(0.4, 1.6, n_out))):
            out['%s_%s.action_scaling' % (env, sc_tag)] = np.asarray(scaling, dtype=np.float64)
            for algo, cls in (('td3', mod.TD3ActorNetwork), ('ddpg', mod.DDPGActorNetwork)):
                net = cls((n_in,), (n_out,), [64, 64], action_scaling=scaling, use_cuda=False)
                net.load_state_dict(base.state_dict())
                with torch.no_grad():
                    out['%s_%s_%s.y' % (algo, env, sc_tag)] = net(torch.from_numpy(x)).numpy()
    np.savez_compressed(args.out, **out)
    print(args.out, os.path.getsize(args.out), 'bytes,', len(out), 'arrays')


if __name__ == '__main__':
    main()
