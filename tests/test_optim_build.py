"""CPU-only checks of the third table of rl_on_manifold_amd/build.py: ADDITIONS holds libatacom_optim.so, build(), stale() and
sources() take its key, its include closure follows `../` into csrc/, and the two pinned tables are as they were
(tests/test_build_table.py, tests/test_fit_build.py).  ADDITIONS is the open table: rows may be appended, so nothing here
counts its rows -- a row is checked for what it is, and the table for holding it.  No source is edited."""
import importlib
import os

import abi_tools as abi

OWN = {'atacom_optim.h', 'atacom_optim.hip', 'atacom_optim_capi.cpp', 'atacom_optim_hip.h'}


def test_the_optim_row_and_what_follows_from_its_key():
    from rl_on_manifold_amd import build
    assert 'optim' in build.ADDITIONS and 'may be appended' in build.__doc__
    t = build.ADDITIONS['optim']
    assert isinstance(t, build.Target) and all(isinstance(r, build.Target) for r in build.ADDITIONS.values())
    assert os.path.basename(t.lib) == 'libatacom_optim.so' or os.environ.get('ATACOM_OPTIM_LIB_OUT')
    assert t.dir == os.path.join(build.CSRC, 'optim') and t.units == ['atacom_optim.hip', 'atacom_optim_capi.cpp'] and t.tuning is False
    assert sorted(f for f in os.listdir(t.dir) if f.endswith(('.h', '.hip', '.cpp'))) == ['atacom_optim.h', 'atacom_optim.hip',
                                                                                        'atacom_optim_capi.cpp']
    assert build.UNIT_FLAGS['atacom_optim.hip'] == ['-ffp-contract=off']
    n = build.naming('optim')
    assert (n.file, n.env, n.symbols, n.binding) == ('libatacom_optim.so', 'ATACOM_OPTIM_LIB', 'atacom_optim_', '_lib_optim')
    binding = importlib.import_module('rl_on_manifold_amd.' + n.binding)
    if not os.environ.get('ATACOM_OPTIM_LIB') and not os.environ.get('ATACOM_OPTIM_LIB_OUT'):
        assert binding.LIB_PATH == t.lib == os.path.join(build.HERE, 'libatacom_optim.so')
    # a key names one row of one table
    assert not set(build.ADDITIONS) & (set(build.TARGETS) | set(build.EXTENSIONS))


def test_the_include_closure_is_its_own_files_and_the_scaffolding():
    from rl_on_manifold_amd import build
    src = build.sources('optim')
    assert src == build.sources(build.ADDITIONS['optim'])
    assert all(os.path.isabs(p) and os.path.isfile(p) for p in src)
    assert {os.path.basename(p) for p in src} == OWN | {'atacom_capi_common.h'}
    where = {os.path.basename(p): os.path.dirname(p) for p in src}
    assert where['atacom_capi_common.h'] == build.CSRC and where['atacom_optim_hip.h'] == abi.INCLUDE
    # it lends nothing: editing its files makes no other library stale
    for table in (build.TARGETS, build.EXTENSIONS):
        for name, t in table.items():
            assert not OWN & {os.path.basename(p) for p in build.sources(t)}, name


def test_a_touched_file_of_its_own_makes_only_optim_stale(monkeypatch):
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
        assert [n for n in every if build.stale(n)] == ['optim'], name
    touched[:] = ['atacom_capi_common.h']
    assert build.stale('optim') and build.stale('fit') and build.stale('returns')
    for other in ('atacom_policy.h', 'atacom_fit.hip', 'atacom_fit_hip.h', 'atacom_evaluate_hip.h', 'atacom_hip.h'):
        touched[:] = [other]
        assert not build.stale('optim'), other


def test_the_pinned_tables_are_unchanged_and_build_additions_builds_the_row():
    from rl_on_manifold_amd import build
    assert list(build.TARGETS) == ['hip', 'point', 'point_policy', 'point_compact', 'point_vec', 'returns', 'evaluate']
    assert list(build.EXTENSIONS) == ['fit']
    assert 'optim' not in build.TARGETS and 'optim' not in build.EXTENSIONS
    more = build.build_additions(verbose=False)
    assert more == [t.lib for t in build.ADDITIONS.values()] and build.ADDITIONS['optim'].lib in more
    assert all(os.path.isfile(p) for p in more)
    assert build.build('optim', verbose=False) == build.ADDITIONS['optim'].lib
    assert 'build_additions' in open(os.path.join(abi.ROOT, '__graft_entry__.py')).read()
