"""CPU-only checks of the 'soft' row of build.ADDITIONS, the open table of rl_on_manifold_amd/build.py: the row is there with its
own properties, build(), stale() and sources() take its key, its include closure is exactly its own files, the borrowed headers
(the network's LDS layout, the host description, the scaffolding, the view type) and the three headers of csrc/mlp/ (the forward
pass, the backward pass and the view checks), with nothing of fit, trust, optim, offpolicy or offgrad, a touched file of its own makes no other
library stale, a touched header of csrc/mlp/ exactly the libraries that share it, its unit is compiled without contraction, and
the two pinned tables are as they were.  Nothing here counts the rows of ADDITIONS.  No source is edited."""
import importlib
import os

import abi_tools as abi

OWN = {'atacom_soft.h', 'atacom_soft.hip', 'atacom_soft_capi.cpp', 'atacom_soft_hip.h'}
BORROWED = {'atacom_policy.h', 'atacom_quad.h', 'atacom_linalg.h', 'atacom_mlp_host.h', 'atacom_capi_common.h', 'atacom_hip.h',
            'atacom_evaluate_hip.h'}
# csrc/mlp/: the backward pass it shares with fit, trust and offgrad; the forward pass in front of it, which it shares with
# offgrad; the view checks, which offpolicy includes too
SHARED = {'atacom_mlp_backward.h': ['fit', 'trust', 'offgrad', 'soft'], 'atacom_mlp_forward.h': ['offgrad', 'soft'],
          'atacom_view_checks.h': ['fit', 'trust', 'offpolicy', 'offgrad', 'soft']}


def test_the_soft_row_and_what_follows_from_its_key():
    from rl_on_manifold_amd import build
    assert 'soft' in build.ADDITIONS and 'may be appended' in build.__doc__ and 'libatacom_soft.so' in build.__doc__
    assert "\n'soft': a SAC update (include/atacom_soft_hip.h)" in open(build.__file__).read()      # the table's docstring
    t = build.ADDITIONS['soft']
    assert isinstance(t, build.Target)
    assert os.path.basename(t.lib) == 'libatacom_soft.so' or os.environ.get('ATACOM_SOFT_LIB_OUT')
    assert t.dir == os.path.join(build.CSRC, 'soft') and t.units == ['atacom_soft.hip', 'atacom_soft_capi.cpp']
    assert t.tuning is False
    assert sorted(f for f in os.listdir(t.dir) if f.endswith(('.h', '.hip', '.cpp'))) == ['atacom_soft.h', 'atacom_soft.hip',
                                                                                        'atacom_soft_capi.cpp']
    n = build.naming('soft')
    assert (n.file, n.env, n.symbols, n.binding) == ('libatacom_soft.so', 'ATACOM_SOFT_LIB', 'atacom_soft_', '_lib_soft')
    binding = importlib.import_module('rl_on_manifold_amd.' + n.binding)
    if not os.environ.get('ATACOM_SOFT_LIB') and not os.environ.get('ATACOM_SOFT_LIB_OUT'):
        assert binding.LIB_PATH == t.lib == os.path.join(build.HERE, 'libatacom_soft.so')
    assert not set(build.ADDITIONS) & (set(build.TARGETS) | set(build.EXTENSIONS))
    assert list(build.ADDITIONS).index('soft') > list(build.ADDITIONS).index('offgrad')          # appended
    # the row arithmetic is individually rounded operations: no contraction in its kernel unit
    assert build.UNIT_FLAGS['atacom_soft.hip'] == ['-ffp-contract=off']


def test_the_include_closure_is_its_own_files_and_the_borrowed_headers():
    from rl_on_manifold_amd import build
    src = build.sources('soft')
    assert src == build.sources(build.ADDITIONS['soft'])
    assert all(os.path.isabs(p) and os.path.isfile(p) for p in src)
    assert {os.path.basename(p) for p in src} == OWN | BORROWED | set(SHARED)
    where = {os.path.basename(p): os.path.dirname(p) for p in src}
    for name in ('atacom_policy.h', 'atacom_capi_common.h', 'atacom_mlp_host.h'):
        assert where[name] == build.CSRC, name
    assert where['atacom_soft_hip.h'] == abi.INCLUDE and where['atacom_evaluate_hip.h'] == abi.INCLUDE
    for name in SHARED:
        assert where[name] == os.path.join(build.CSRC, 'mlp'), name
    # nothing of the gradient, trust-region, optimiser and off-policy libraries, and it lends nothing
    assert not any(os.path.basename(d) in ('fit', 'trust', 'optim', 'offpolicy', 'offgrad') for d in where.values())
    assert not any(w in name for name in where for w in ('fit', 'trust', 'optim', 'offpolicy', 'offgrad'))
    for table in (build.TARGETS, build.EXTENSIONS, build.ADDITIONS):
        for name, t in table.items():
            if name != 'soft':
                assert not OWN & {os.path.basename(p) for p in build.sources(t)}, name


def test_a_touched_file_of_its_own_makes_only_soft_stale(monkeypatch):
    from rl_on_manifold_amd import build
    tables = (build.TARGETS, build.EXTENSIONS, build.ADDITIONS)
    libs = [t.lib for table in tables for t in table.values()]
    touched = []
    real_exists = os.path.exists
    monkeypatch.setattr(build.os.path, 'exists', lambda p: p in libs or real_exists(p))
    monkeypatch.setattr(build.os.path, 'getmtime', lambda p: 2.0 if os.path.basename(p) in touched else 1.0)
    every = [name for table in tables for name in table]
    assert not any(build.stale(n) for n in every)
    for name in sorted(OWN):
        touched[:] = [name]
        assert [n for n in every if build.stale(n)] == ['soft'], name
    touched[:] = ['atacom_policy.h']
    assert build.stale('soft') and build.stale('offgrad') and not build.stale('optim')
    touched[:] = ['atacom_evaluate_hip.h']
    assert build.stale('soft')
    for other in ('atacom_fit.hip', 'atacom_fit_hip.h', 'atacom_trust.hip', 'atacom_optim.hip', 'atacom_optim_hip.h', 'atacom_returns.hip',
                  'atacom_evaluate.hip', 'atacom_offpolicy.hip', 'atacom_offpolicy.h', 'atacom_offpolicy_hip.h', 'atacom_offgrad.hip',
                  'atacom_offgrad.h', 'atacom_offgrad_hip.h'):
        touched[:] = [other]
        assert not build.stale('soft'), other
    # the shared headers of csrc/mlp/: exactly the libraries named above and nothing else
    for name, users in sorted(SHARED.items()):
        touched[:] = [name]
        assert [n for n in every if build.stale(n)] == users, name


def test_the_pinned_tables_are_unchanged_and_build_additions_builds_the_row():
    from rl_on_manifold_amd import build
    assert list(build.TARGETS) == ['hip', 'point', 'point_policy', 'point_compact', 'point_vec', 'returns', 'evaluate']
    assert list(build.EXTENSIONS) == ['fit']
    assert list(build.ADDITIONS)[:4] == ['optim', 'trust', 'offpolicy', 'offgrad']
    more = build.build_additions(verbose=False)
    assert build.ADDITIONS['soft'].lib in more and all(os.path.isfile(p) for p in more)
    assert build.build('soft', verbose=False) == build.ADDITIONS['soft'].lib
