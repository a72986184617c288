"""CPU-only checks of the second table of rl_on_manifold_amd/build.py: EXTENSIONS holds libatacom_fit.so beside the seven rows
of TARGETS, build(), stale() and sources() take its key, its include closure follows `../` into csrc/, and the table of the
seven is as it was (tests/test_build_table.py pins it).  No source is edited."""
import importlib
import os

import abi_tools as abi

OWN = {'atacom_fit.h', 'atacom_fit.hip', 'atacom_fit_capi.cpp', 'atacom_fit_hip.h'}
# csrc/mlp/: headers it shares with libatacom_trust.so, libatacom_offgrad.so and libatacom_soft.so -- the view checks with
# libatacom_offpolicy.so too
SHARED = {'atacom_mlp_backward.h': ['fit', 'trust', 'offgrad', 'soft'], 'atacom_view_checks.h': ['fit', 'trust', 'offpolicy', 'offgrad', 'soft']}


def test_extensions_is_the_one_row():
    from rl_on_manifold_amd import build
    assert list(build.EXTENSIONS) == ['fit']
    t = build.EXTENSIONS['fit']
    assert isinstance(t, build.Target)
    assert os.path.basename(t.lib) == 'libatacom_fit.so' or os.environ.get('ATACOM_FIT_LIB_OUT')
    assert t.dir == os.path.join(build.CSRC, 'fit') and t.units == ['atacom_fit.hip', 'atacom_fit_capi.cpp'] and t.tuning is False
    assert sorted(f for f in os.listdir(t.dir) if f.endswith(('.h', '.hip', '.cpp'))) == ['atacom_fit.h', 'atacom_fit.hip', 'atacom_fit_capi.cpp']
    n = build.naming('fit')
    assert (n.file, n.env, n.symbols, n.binding) == ('libatacom_fit.so', 'ATACOM_FIT_LIB', 'atacom_fit_', '_lib_fit')
    binding = importlib.import_module('rl_on_manifold_amd.' + n.binding)
    if not os.environ.get('ATACOM_FIT_LIB') and not os.environ.get('ATACOM_FIT_LIB_OUT'):
        assert binding.LIB_PATH == t.lib == os.path.join(build.HERE, 'libatacom_fit.so')
    assert not set(build.EXTENSIONS) & set(build.TARGETS)


def test_the_include_closure_follows_the_borrowed_headers_into_csrc():
    from rl_on_manifold_amd import build
    src = build.sources('fit')
    assert src == build.sources(build.EXTENSIONS['fit'])
    assert all(os.path.isabs(p) and os.path.isfile(p) for p in src)
    names = {os.path.basename(p) for p in src}
    assert OWN | {'atacom_policy.h', 'atacom_mlp_host.h', 'atacom_capi_common.h'} <= names
    assert names == OWN | set(SHARED) | {'atacom_policy.h', 'atacom_quad.h', 'atacom_linalg.h', 'atacom_mlp_host.h', 'atacom_capi_common.h',
                                    'atacom_hip.h', 'atacom_evaluate_hip.h'}
    # the borrowed files are the ones directly inside csrc/ and include/, not copies
    where = {os.path.basename(p): os.path.dirname(p) for p in src}
    assert where['atacom_policy.h'] == build.CSRC and where['atacom_fit_hip.h'] == abi.INCLUDE
    for name in SHARED:
        assert where[name] == os.path.join(build.CSRC, 'mlp'), name
    # it lends nothing: editing its files makes none of the seven stale
    for name, t in build.TARGETS.items():
        assert not OWN & {os.path.basename(p) for p in build.sources(t)}, name


def test_a_touched_file_makes_fit_stale_and_its_own_files_only_fit(monkeypatch):
    from rl_on_manifold_amd import build
    libs = [t.lib for t in list(build.TARGETS.values()) + list(build.EXTENSIONS.values())]
    touched = []
    real_exists = os.path.exists
    monkeypatch.setattr(build.os.path, 'exists', lambda p: p in libs or real_exists(p))
    monkeypatch.setattr(build.os.path, 'getmtime', lambda p: 2.0 if os.path.basename(p) in touched else 1.0)
    every = list(build.TARGETS) + list(build.EXTENSIONS)
    assert [build.stale(n) for n in every] == [False] * 8
    for name in sorted(OWN):
        touched[:] = [name]
        assert [n for n in every if build.stale(n)] == ['fit'], name
    touched[:] = ['atacom_policy.h']
    assert build.stale('fit') and build.stale('evaluate') and not build.stale('returns')
    touched[:] = ['atacom_evaluate_hip.h']                 # the view struct is borrowed from the evaluate library's header
    assert [n for n in every if build.stale(n)] == ['evaluate', 'fit']
    touched[:] = ['atacom_returns.hip']
    assert not build.stale('fit')
    # the shared headers of csrc/mlp/: exactly the libraries named above, none of the seven and not optim
    libs += [t.lib for t in build.ADDITIONS.values()]
    for name, users in sorted(SHARED.items()):
        touched[:] = [name]
        assert [n for n in every + list(build.ADDITIONS) if build.stale(n)] == users, name


def test_the_seven_are_still_the_seven_and_build_extensions_builds_the_rest():
    from rl_on_manifold_amd import build
    assert len(build.TARGETS) == 7 and 'fit' not in build.TARGETS
    libs = build.build_all(verbose=False)
    assert libs == [t.lib for t in build.TARGETS.values()] and len(libs) == 7
    more = build.build_extensions(verbose=False)
    assert more == [build.EXTENSIONS['fit'].lib] and os.path.isfile(more[0])
    assert build.build('fit', verbose=False) == more[0]
