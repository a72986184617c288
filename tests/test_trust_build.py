"""CPU-only checks of the 'trust' row of build.ADDITIONS, the open table of rl_on_manifold_amd/build.py: the row is there with its
own properties, build(), stale() and sources() take its key, its include closure follows `../` into csrc/ (the borrowed network,
host description, scaffolding and view type), a touched file of its own makes no other library stale, and the two pinned tables
are as they were.  Nothing here counts the rows of ADDITIONS.  No source is edited."""
import importlib
import os

import abi_tools as abi

OWN = {'atacom_trust.h', 'atacom_trust.hip', 'atacom_trust_capi.cpp', 'atacom_trust_hip.h'}
BORROWED = {'atacom_policy.h', 'atacom_quad.h', 'atacom_linalg.h', 'atacom_mlp_host.h', 'atacom_capi_common.h', 'atacom_hip.h',
            'atacom_evaluate_hip.h'}
# csrc/mlp/: headers it shares with libatacom_fit.so, libatacom_offgrad.so and libatacom_soft.so -- the view checks with
# libatacom_offpolicy.so too
SHARED = {'atacom_mlp_backward.h': ['fit', 'trust', 'offgrad', 'soft'], 'atacom_view_checks.h': ['fit', 'trust', 'offpolicy', 'offgrad', 'soft']}


def test_the_trust_row_and_what_follows_from_its_key():
    from rl_on_manifold_amd import build
    assert 'trust' in build.ADDITIONS and 'may be appended' in build.__doc__ and 'libatacom_trust.so' in build.__doc__
    t = build.ADDITIONS['trust']
    assert isinstance(t, build.Target)
    assert os.path.basename(t.lib) == 'libatacom_trust.so' or os.environ.get('ATACOM_TRUST_LIB_OUT')
    assert t.dir == os.path.join(build.CSRC, 'trust') and t.units == ['atacom_trust.hip', 'atacom_trust_capi.cpp'] and t.tuning is False
    assert sorted(f for f in os.listdir(t.dir) if f.endswith(('.h', '.hip', '.cpp'))) == ['atacom_trust.h', 'atacom_trust.hip',
                                                                                        'atacom_trust_capi.cpp']
    n = build.naming('trust')
    assert (n.file, n.env, n.symbols, n.binding) == ('libatacom_trust.so', 'ATACOM_TRUST_LIB', 'atacom_trust_', '_lib_trust')
    binding = importlib.import_module('rl_on_manifold_amd.' + n.binding)
    if not os.environ.get('ATACOM_TRUST_LIB') and not os.environ.get('ATACOM_TRUST_LIB_OUT'):
        assert binding.LIB_PATH == t.lib == os.path.join(build.HERE, 'libatacom_trust.so')
    assert not set(build.ADDITIONS) & (set(build.TARGETS) | set(build.EXTENSIONS))


def test_the_include_closure_is_its_own_files_and_the_borrowed_headers():
    from rl_on_manifold_amd import build
    src = build.sources('trust')
    assert src == build.sources(build.ADDITIONS['trust'])
    assert all(os.path.isabs(p) and os.path.isfile(p) for p in src)
    assert {os.path.basename(p) for p in src} == OWN | BORROWED | set(SHARED)
    where = {os.path.basename(p): os.path.dirname(p) for p in src}
    assert where['atacom_policy.h'] == build.CSRC and where['atacom_capi_common.h'] == build.CSRC
    for name in SHARED:
        assert where[name] == os.path.join(build.CSRC, 'mlp'), name
    assert where['atacom_trust_hip.h'] == abi.INCLUDE and where['atacom_evaluate_hip.h'] == abi.INCLUDE
    # it borrows nothing of the gradient library's own, and lends nothing
    assert not any('fit' in name for name in where)
    for table in (build.TARGETS, build.EXTENSIONS, build.ADDITIONS):
        for name, t in table.items():
            if name != 'trust':
                assert not OWN & {os.path.basename(p) for p in build.sources(t)}, name


def test_a_touched_file_of_its_own_makes_only_trust_stale(monkeypatch):
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
        assert [n for n in every if build.stale(n)] == ['trust'], name
    touched[:] = ['atacom_policy.h']
    assert build.stale('trust') and build.stale('fit') and build.stale('evaluate') and not build.stale('optim')
    touched[:] = ['atacom_evaluate_hip.h']
    assert build.stale('trust')
    for other in ('atacom_fit.hip', 'atacom_fit_hip.h', 'atacom_fit.h', 'atacom_optim.hip', 'atacom_returns.hip'):
        touched[:] = [other]
        assert not build.stale('trust'), other
    # the shared headers of csrc/mlp/: exactly the libraries named above, none of the seven and not optim
    for name, users in sorted(SHARED.items()):
        touched[:] = [name]
        assert [n for n in every if build.stale(n)] == users, name


def test_the_pinned_tables_are_unchanged_and_build_additions_builds_the_row():
    from rl_on_manifold_amd import build
    assert list(build.TARGETS) == ['hip', 'point', 'point_policy', 'point_compact', 'point_vec', 'returns', 'evaluate']
    assert list(build.EXTENSIONS) == ['fit']
    more = build.build_additions(verbose=False)
    assert build.ADDITIONS['trust'].lib in more and all(os.path.isfile(p) for p in more)
    assert build.build('trust', verbose=False) == build.ADDITIONS['trust'].lib
