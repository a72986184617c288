"""Build the package's shared libraries in-tree with hipcc for gfx950 (no GPU needed: hipcc cross-compiles).

    python -m rl_on_manifold_amd.build [--force]

TARGETS below describes each library: libatacom_hip.so (the air-hockey and circle tasks), libatacom_point.so (the
collision-avoidance task), libatacom_point_policy.so (its rollout with the actor network in the kernel),
libatacom_point_compact.so (that rollout in the compact record format) and libatacom_point_vec.so (the task's masked step and
checkpoint); beside the table, libatacom_returns.so (advantages and episode returns of a finished collection; its sources are in
csrc_returns/).  A library is one translation unit per group of kernels (they compile in parallel) plus its C-ABI host file, linked into
rl_on_manifold_amd/.  The .so files are git-ignored.
"""
import os
import subprocess
import sys
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
ARCH = 'gfx950'
FLAGS = ['--offload-arch=' + ARCH, '-O3', '-std=c++17', '-fPIC', '-Wall', '-Wno-unused-function'] + \
    os.environ.get('ATACOM_HIPCC_FLAGS', '').split()
UNITS = ['atacom_iiwa.hip', 'atacom_iiwa_group.hip', 'atacom_iiwa_f64.hip', 'atacom_noise_iiwa.hip', 'atacom_noise_iiwa_f64.hip', 'atacom_iiwa_dyn.hip',
         'atacom_iiwa_dyn_f64.hip', 'atacom_iiwa_dyn_chart.hip', 'atacom_chart_iiwa.hip', 'atacom_planar.hip',
         'atacom_noise_planar.hip', 'atacom_chart.hip', 'atacom_circle.hip',
         'atacom_capi.cpp']           # longest first: the pool runs min(cores, units) compilers
# per-unit extra flags.  atacom_iiwa_group.hip holds the 4- / 8-lane float32 iiwa kernels alone so that they can take the
# iterative-ilp scheduler (-1.0 % on the headline step, profiles/r05_ab_sched.log) without the lane kernels of the same source
# paying for it (+29 % on the lane rollout kernel, r04_ab_sched_iterative_ilp.log; the option also crashes the compiler on
# float64 instantiations).  (-amdgpu-sched-strategy=max-ilp was tried per unit in round 1 -- planar step kernel -4 %, planar
# policy-rollout kernel +19 %, iiwa quad kernel +8 % -- and dropped, profiles/r01_lanes_vs_batch.md; round 5: +0.7 % on the headline)
# atacom_returns.hip: the fused multiply-adds of its recurrences are the explicit ones (include/atacom_returns_hip.h); the compiler
# adds none
UNIT_FLAGS = {'atacom_iiwa_group.hip': ['-mllvm', '-amdgpu-sched-strategy=iterative-ilp'],
              'atacom_returns.hip': ['-ffp-contract=off']}


def _include(name):
    return os.path.join(os.path.dirname(HERE), 'include', name)


# One description per library.  `private`: the headers of csrc/ that belong to it alone; `feeds`: the libraries whose
# private headers it includes as well; `headers`: the public headers it depends on; `tuning`: whether it takes the
# ATACOM_ONLY_UNITS / kept-object path below.  A new library is a new entry here.
Target = namedtuple('Target', 'lib units private feeds headers tuning')


def _lib_out(env, name):
    return os.environ.get(env) or os.path.join(HERE, name)


TARGETS = {
    'hip': Target(_lib_out('ATACOM_LIB_OUT', 'libatacom_hip.so'), UNITS, (), (), ('atacom_hip.h',), True),
    # The collision-avoidance task (PointReachAtacom) is a library of its own (include/atacom_point_hip.h): its kernels stay
    # out of the main library's census and it shares only headers (the solver of atacom_linalg.h, the host scaffolding of
    # atacom_capi_common.h) with it.
    'point': Target(_lib_out('ATACOM_POINT_LIB_OUT', 'libatacom_point.so'), ['atacom_point.hip', 'atacom_point_capi.cpp'],
                    ('atacom_point.h', 'atacom_point_ops.h', 'atacom_point_handle.h'), (), ('atacom_point_hip.h',), False),
    # The task's rollout with the actor network evaluated in the kernel is a third library (include/atacom_point_policy_hip.h):
    # it borrows the handles of libatacom_point.so (csrc/atacom_point_handle.h) and keeps the kernel census of the other
    # two as it is.
    'point_policy': Target(_lib_out('ATACOM_POINT_POLICY_LIB_OUT', 'libatacom_point_policy.so'),
                           ['atacom_point_policy.hip', 'atacom_point_policy_capi.cpp'],
                           ('atacom_point_policy.h', 'atacom_point_policy_ops.h'), ('point',),
                           ('atacom_hip.h', 'atacom_point_hip.h', 'atacom_point_policy_hip.h'), False),
    # The task's rollout in the compact record format is a fourth library (include/atacom_point_compact_hip.h): it borrows the
    # handles of libatacom_point.so and the network, LDS layout and argument checks of libatacom_point_policy.so, and keeps
    # the kernel census of the other three as it is.
    'point_compact': Target(_lib_out('ATACOM_POINT_COMPACT_LIB_OUT', 'libatacom_point_compact.so'),
                            ['atacom_point_compact.hip', 'atacom_point_compact_capi.cpp'],
                            ('atacom_point_compact.h', 'atacom_point_compact_ops.h'), ('point', 'point_policy'),
                            ('atacom_hip.h', 'atacom_point_hip.h', 'atacom_point_policy_hip.h', 'atacom_point_compact_hip.h'),
                            False),
    # The task's masked step and checkpoint are a fifth library (include/atacom_point_vec_hip.h): it borrows the handles and the
    # environment (atacom_point.h) of libatacom_point.so and keeps the kernel census of the other four as it is.
    'point_vec': Target(_lib_out('ATACOM_POINT_VEC_LIB_OUT', 'libatacom_point_vec.so'),
                        ['atacom_point_vec.hip', 'atacom_point_vec_capi.cpp'],
                        ('atacom_point_vec.h', 'atacom_point_vec_ops.h'), ('point',),
                        ('atacom_point_hip.h', 'atacom_point_vec_hip.h'), False),
}
_MAIN, _POINT, _POINT_POLICY, _POINT_COMPACT, _POINT_VEC = (TARGETS[k] for k in ('hip', 'point', 'point_policy', 'point_compact',
                                                                                 'point_vec'))
LIB, LIB_POINT, LIB_POINT_POLICY, LIB_POINT_COMPACT = _MAIN.lib, _POINT.lib, _POINT_POLICY.lib, _POINT_COMPACT.lib
LIB_POINT_VEC, UNITS_POINT_VEC = _POINT_VEC.lib, _POINT_VEC.units
UNITS_POINT, UNITS_POINT_POLICY, UNITS_POINT_COMPACT = _POINT.units, _POINT_POLICY.units, _POINT_COMPACT.units


# The post-processing of a collection (include/atacom_returns_hip.h) is a sixth library that belongs to no environment: it is
# NOT an entry of TARGETS and its sources live in a directory of their own, so that _sources() of the five libraries above never
# lists them.  It shares one header with them, the host scaffolding of csrc/atacom_capi_common.h.
CSRC_RETURNS = os.path.join(HERE, 'csrc_returns')
_RETURNS = Target(_lib_out('ATACOM_RETURNS_LIB_OUT', 'libatacom_returns.so'), ['atacom_returns.hip', 'atacom_returns_capi.cpp'],
                  (), (), ('atacom_returns_hip.h',), False)
LIB_RETURNS, UNITS_RETURNS = _RETURNS.lib, _RETURNS.units


def _sources_returns():
    """Everything in csrc_returns/, the shared host scaffolding and the public header."""
    own = [os.path.join(CSRC_RETURNS, f) for f in os.listdir(CSRC_RETURNS) if f.endswith(('.h', '.hip', '.cpp'))]
    return own + [os.path.join(CSRC, 'atacom_capi_common.h')] + [_include(h) for h in _RETURNS.headers]


def _sources(target=_MAIN):
    """What a library is rebuilt for: its own units, every header of csrc/ that is not private to a library that does not
    feed it, and its public headers."""
    foreign = {h for name, t in TARGETS.items() if t is not target and name not in target.feeds for h in t.private}
    out = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f in target.units or (f.endswith('.h') and f not in foreign)]
    return out + [_include(h) for h in target.headers]


def _sources_point():
    return _sources(_POINT)


def _sources_point_policy():
    return _sources(_POINT_POLICY)


def _sources_point_compact():
    return _sources(_POINT_COMPACT)


def _sources_point_vec():
    return _sources(_POINT_VEC)


def _stale(target):
    if not os.path.exists(target.lib):
        return True
    t = os.path.getmtime(target.lib)
    sources = _sources_returns() if target is _RETURNS else _sources(target)
    return any(os.path.getmtime(p) > t for p in sources)


def needs_build():
    return _stale(_MAIN)


def needs_build_point():
    return _stale(_POINT)


def needs_build_point_policy():
    return _stale(_POINT_POLICY)


def needs_build_point_compact():
    return _stale(_POINT_COMPACT)


def needs_build_point_vec():
    return _stale(_POINT_VEC)


def needs_build_returns():
    return _stale(_RETURNS)


# kernel-tuning builds: ATACOM_KEEP_OBJ=1 keeps the objects of a build; ATACOM_ONLY_UNITS=a.hip,b.hip then recompiles only
# those units (with ATACOM_HIPCC_FLAGS applied to them alone) and links against the kept objects of the others
ONLY = [u for u in os.environ.get('ATACOM_ONLY_UNITS', '').split(',') if u]


def _compile(target, unit, csrc=CSRC):
    src = os.path.join(csrc, unit)
    tag = os.environ.get('ATACOM_OBJ_TAG', '')
    obj = os.path.join(csrc, os.path.splitext(unit)[0] + tag + '.o')
    if ONLY and target.tuning and unit not in ONLY:
        kept = os.path.join(csrc, os.path.splitext(unit)[0] + os.environ.get('ATACOM_BASE_TAG', '_keep') + '.o')
        if not os.path.exists(kept):
            raise RuntimeError('ATACOM_ONLY_UNITS needs the kept object %s (build once with ATACOM_KEEP_OBJ=1 ATACOM_OBJ_TAG=_keep)' % kept)
        return kept
    cmd = [HIPCC] + FLAGS + UNIT_FLAGS.get(unit, []) + (['-x', 'hip'] if unit.endswith('.cpp') else []) + ['-c', src, '-o', obj]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError('hipcc failed for %s:\n%s\n%s' % (unit, ' '.join(cmd), r.stderr[-4000:]))
    return obj


# The kernels run at the edge of the register file and two compiler defects have been met there (a miscompiled float64
# instantiation in round 1; register copies under a narrowed exec mask, profiles/r06_exec_mask_copies.md).  The shipped code is
# validated with THIS compiler; another one is not refused -- tests/test_kernel_resources.py audits whatever it produced --
# but it is named.
VALIDATED_HIPCC = 'HIP version: 7.2'


def _hipcc_version():
    try:
        out = subprocess.run([HIPCC, '--version'], capture_output=True, text=True).stdout
        return next((ln.strip() for ln in out.splitlines() if ln.startswith('HIP version')), out.strip()[:60])
    except OSError as e:
        return 'unavailable (%s)' % e


def _build(target, force, verbose, csrc=CSRC):
    if not force and not _stale(target):
        return target.lib
    if verbose:
        print('[atacom] building %s for %s ...' % (os.path.basename(target.lib), ARCH), flush=True)
    with ThreadPoolExecutor(max_workers=min(len(target.units), os.cpu_count() or 4)) as ex:
        objs = list(ex.map(lambda u: _compile(target, u, csrc), target.units))
    cmd = [HIPCC, '--offload-arch=' + ARCH, '-shared', '-fPIC', '-o', target.lib] + objs
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError('link failed:\n%s\n%s' % (' '.join(cmd), r.stderr[-4000:]))
    if not os.environ.get('ATACOM_KEEP_OBJ'):
        for o in objs:
            if not (ONLY and target.tuning and o.endswith(os.environ.get('ATACOM_BASE_TAG', '_keep') + '.o')):
                os.remove(o)
    return target.lib


def build(force=False, verbose=True):
    """libatacom_hip.so: fourteen units, a few minutes."""
    if force or needs_build():
        ver = _hipcc_version()
        if not ver.startswith(VALIDATED_HIPCC):
            print('[atacom] WARNING: building with "%s"; the kernels were validated with hipcc 7.2 -- run the code-object audits '
                  '(python -m pytest tests/test_kernel_resources.py) and the GPU suite before trusting this build' % ver, flush=True)
    return _build(_MAIN, force, verbose)


def build_point(force=False, verbose=True):
    """libatacom_point.so: two units, a few seconds."""
    return _build(_POINT, force, verbose)


def build_point_policy(force=False, verbose=True):
    """libatacom_point_policy.so: two units; the four policy kernels take about a minute."""
    return _build(_POINT_POLICY, force, verbose)


def build_point_compact(force=False, verbose=True):
    """libatacom_point_compact.so: two units; the eight compact kernels take about a minute."""
    return _build(_POINT_COMPACT, force, verbose)


def build_point_vec(force=False, verbose=True):
    """libatacom_point_vec.so: two units, a few seconds."""
    return _build(_POINT_VEC, force, verbose)


def build_returns(force=False, verbose=True):
    """libatacom_returns.so: two units, a few seconds."""
    return _build(_RETURNS, force, verbose, CSRC_RETURNS)


if __name__ == '__main__':
    for _b in (build, build_point, build_point_policy, build_point_compact, build_point_vec, build_returns):
        _b(force='--force' in sys.argv)
    for _t in list(TARGETS.values()) + [_RETURNS]:
        print(_t.lib)
