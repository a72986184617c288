"""CPU-only checks of the 'offstep' row of build.ADDITIONS, the open table of rl_on_manifold_amd/build.py: the row is there with
its own properties, build(), stale() and sources() take its key, its include closure is exactly its own files and the host
scaffolding -- nothing of csrc/mlp/ and nothing of another library's directory -- a touched file of its own makes no other library
stale, its unit is compiled without contraction, and the two pinned tables are as they were.  Nothing here counts the rows of
ADDITIONS.  No source is edited."""
import importlib
import os

import abi_tools as abi

OWN = {'atacom_offstep.h', 'atacom_offstep.hip', 'atacom_offstep_capi.cpp', 'atacom_offstep_hip.h'}


def test_the_offstep_row_and_what_follows_from_its_key():
    from rl_on_manifold_amd import build
    assert 'offstep' in build.ADDITIONS and 'may be appended' in build.__doc__ and 'libatacom_offstep.so' in build.__doc__
    assert "\n'offstep': the Adam step of an off-policy update" in open(build.__file__).read()      # the table's docstring
    t = build.ADDITIONS['offstep']
    assert isinstance(t, build.Target)
    assert os.path.basename(t.lib) == 'libatacom_offstep.so' or os.environ.get('ATACOM_OFFSTEP_LIB_OUT')
    assert t.dir == os.path.join(build.CSRC, 'offstep') and t.units == ['atacom_offstep.hip', 'atacom_offstep_capi.cpp']
    assert t.tuning is False
    assert sorted(f for f in os.listdir(t.dir) if f.endswith(('.h', '.hip', '.cpp'))) == ['atacom_offstep.h', 'atacom_offstep.hip',
                                                                                        'atacom_offstep_capi.cpp']
    n = build.naming('offstep')
    assert (n.file, n.env, n.symbols, n.binding) == ('libatacom_offstep.so', 'ATACOM_OFFSTEP_LIB', 'atacom_offstep_', '_lib_offstep')
    binding = importlib.import_module('rl_on_manifold_amd.' + n.binding)
    if not os.environ.get('ATACOM_OFFSTEP_LIB') and not os.environ.get('ATACOM_OFFSTEP_LIB_OUT'):
        assert binding.LIB_PATH == t.lib == os.path.join(build.HERE, 'libatacom_offstep.so')
    assert not set(build.ADDITIONS) & (set(build.TARGETS) | set(build.EXTENSIONS))
    assert list(build.ADDITIONS).index('offstep') > list(build.ADDITIONS).index('soft')          # appended
    # every operation is the individually rounded one of atacom_optim.hip and of the soft update: no contraction
    assert build.UNIT_FLAGS['atacom_offstep.hip'] == ['-ffp-contract=off']


def test_the_include_closure_is_its_own_files_and_the_scaffolding():
    from rl_on_manifold_amd import build
    src = build.sources('offstep')
    assert src == build.sources(build.ADDITIONS['offstep'])
    assert all(os.path.isabs(p) and os.path.isfile(p) for p in src)
    assert {os.path.basename(p) for p in src} == OWN | {'atacom_capi_common.h'}
    where = {os.path.basename(p): os.path.dirname(p) for p in src}
    assert where['atacom_capi_common.h'] == build.CSRC and where['atacom_offstep_hip.h'] == abi.INCLUDE
    assert {where[n] for n in OWN - {'atacom_offstep_hip.h'}} == {os.path.join(build.CSRC, 'offstep')}
    # it lends nothing: no other library reaches one of its files
    for table in (build.TARGETS, build.EXTENSIONS, build.ADDITIONS):
        for name, t in table.items():
            if name != 'offstep':
                assert not OWN & {os.path.basename(p) for p in build.sources(t)}, name


def test_a_touched_file_of_its_own_makes_only_offstep_stale(monkeypatch):
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
        assert [n for n in every if build.stale(n)] == ['offstep'], name
    touched[:] = ['atacom_capi_common.h']
    assert build.stale('offstep') and build.stale('optim') and build.stale('offpolicy')
    for other in ('atacom_policy.h', 'atacom_optim.hip', 'atacom_optim.h', 'atacom_optim_hip.h', 'atacom_offpolicy.hip', 'atacom_offpolicy_hip.h',
                  'atacom_offgrad.hip', 'atacom_offgrad_hip.h', 'atacom_soft.hip', 'atacom_fit_hip.h', 'atacom_evaluate_hip.h', 'atacom_hip.h',
                  'atacom_mlp_backward.h', 'atacom_view_checks.h'):
        touched[:] = [other]
        assert not build.stale('offstep'), other


def test_the_pinned_tables_are_unchanged_and_build_additions_builds_the_row():
    from rl_on_manifold_amd import build
    assert list(build.TARGETS) == ['hip', 'point', 'point_policy', 'point_compact', 'point_vec', 'returns', 'evaluate']
    assert list(build.EXTENSIONS) == ['fit']
    assert list(build.ADDITIONS)[:5] == ['optim', 'trust', 'offpolicy', 'offgrad', 'soft']
    more = build.build_additions(verbose=False)
    assert build.ADDITIONS['offstep'].lib in more and all(os.path.isfile(p) for p in more)
    assert build.build('offstep', verbose=False) == build.ADDITIONS['offstep'].lib
