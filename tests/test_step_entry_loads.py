"""The headline step kernel asks for its kernel arguments in one round trip.

The compiler puts each scalar load of a kernel argument into the basic block that first uses it; the bounds check, the mask
test and the masked-out exit cut the top of `k_step` into blocks, and a wave of `k_step<float, Iiwa, 8, true, false, 0, false>`
made five scalar round trips to the kernel-argument segment, one after the other, in front of its first arithmetic
instruction -- four of them to a 64-byte line that no earlier trip had requested, which a freshly started kernel finds in no
cache.  The kernel now requests every line of the segment, and the pointers its first loads go through, next to the batch
size in the entry block (csrc/atacom_kernels.h: kernarg_request_lines; profiles/step_entry.md).  Read from the code object
inside the built libatacom_hip.so, no GPU needed.

What is walked is the path that the benchmark takes: lanes inside the batch, `mask == nullptr`.  A "trip" is a batch of
`s_load` from the kernel-argument segment closed by `s_waitcnt lgkmcnt(0)`; it "misses" when one of its loads touches a
64-byte line of the segment that no load in front of the previous wait had touched."""
import os
import re
import struct
import subprocess

import pytest

LLVM = '/opt/rocm/lib/llvm/bin'
MAGIC = b'__CLANG_OFFLOAD_BUNDLE__'
KERNEL = 'k_step<float, Iiwa, 8, true, false, 0, false>'

pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, 'llvm-readelf')), reason='needs the ROCm LLVM binutils')

DWORDS = {'dword': 1, 'dwordx2': 2, 'dwordx3': 3, 'dwordx4': 4, 'dwordx8': 8, 'dwordx16': 16}
# floating-point vector arithmetic: what the wave is there for (address arithmetic is integer, compares and moves are not it)
ARITH = re.compile(r'^v_(pk_)?(add|sub|mul|fma|fmac|mac|mad|fmamk|fmaak|max|min|rcp|sqrt|rsq|sin|cos|exp|log)\w*_f(16|32|64)\b')


class Ins:
    def __init__(self, label, text):
        self.label, self.text = label, text
        self.op = text.split()[0] if text else ''


@pytest.fixture(scope='module')
def kernel(tmp_path_factory):
    from rl_on_manifold_amd import build
    return disassemble(build.build(verbose=False), str(tmp_path_factory.mktemp('entry_loads')))


def disassemble(so, tmp):
    """(instructions of the headline kernel in layout order, {label: index}, byte offset of the `mask` argument)"""
    fat = os.path.join(tmp, 'fat.bin')
    subprocess.check_call([os.path.join(LLVM, 'llvm-objcopy'), '--dump-section', '.hip_fatbin=' + fat, so,
                           os.path.join(tmp, 'copy.so')])
    data = open(fat, 'rb').read()
    for m in re.finditer(MAGIC, data):                       # one bundle per translation unit
        p = m.start()
        n_entries = struct.unpack_from('<Q', data, p + 24)[0]
        off = p + 32
        for _ in range(n_entries):
            o, size, id_len = struct.unpack_from('<QQQ', data, off)
            ident = data[off + 24:off + 24 + id_len].decode()
            off += 24 + id_len
            if 'gfx950' not in ident or size == 0:
                continue
            elf = os.path.join(tmp, 'dev%d.elf' % p)
            open(elf, 'wb').write(data[p + o:p + o + size])
            notes = subprocess.run([os.path.join(LLVM, 'llvm-readelf'), '--notes', elf], capture_output=True, text=True,
                                   check=True).stdout
            for blk in notes.split('  - .agpr_count:')[1:]:
                mangled = re.search(r'\.name:\s+(\S+)', blk).group(1)
                if 'k_step' not in mangled:
                    continue
                name = subprocess.run(['c++filt', mangled], capture_output=True, text=True).stdout.strip()
                if re.sub(r'\(.*', '', name).replace('atacom::', '').replace('void ', '') != KERNEL:
                    continue
                args = re.findall(r'\.offset:\s+(\d+)\s+\.size:\s+(\d+)\s+\.value_kind:\s+(\S+)', blk)
                mask_off = max(int(o_) for o_, _, kind in args if kind == 'global_buffer')
                # (the whole code object: with --disassemble-symbols the listing of a kernel ends at its first label)
                dis = subprocess.run([os.path.join(LLVM, 'llvm-objdump'), '-d', '--symbolize-operands', '--no-show-raw-insn',
                                      elf], capture_output=True, text=True, check=True).stdout
                dis = dis[dis.index('<%s>:' % mangled):]
                nxt = re.search(r'^[0-9a-f]+ <(?!L\d+>)[^>]+>:', dis[len(mangled) + 3:], re.M)
                dis = dis[:len(mangled) + 3 + nxt.start()] if nxt else dis
                ins, labels, pending = [], {}, None
                for line in dis.split('\n'):
                    lm = re.match(r'^\s*(?:[0-9a-f]+ )?<(L\d+)>:', line)
                    if lm:
                        pending = lm.group(1)
                        continue
                    text = re.sub(r'//.*', '', line).strip()
                    if not re.match(r'^[sv]_|^(global|buffer|flat|ds|scratch)_', text):
                        continue
                    if pending:
                        labels[pending] = len(ins)
                    ins.append(Ins(pending, text))
                    pending = None
                assert any(i.op == 's_endpgm' for i in ins)
                assert sum(i.op.startswith('v_') for i in ins) > 4000          # the kernel was disassembled
                return ins, labels, mask_off
    raise AssertionError(KERNEL + ' not found in ' + so)


def _kernarg_load(i):
    """(first byte, last byte) of a scalar load from the kernel-argument segment (its pointer arrives in s[0:1]), or None"""
    m = re.match(r'^s_load_(dword(?:x\d+)?)\s+\S+,\s*s\[0:1\],\s*(0x[0-9a-f]+|\d+)', i.text)
    if not m:
        return None
    off = int(m.group(2), 0)
    return off, off + 4 * DWORDS[m.group(1)] - 1


def _target(i):
    m = re.search(r'<?(L\d+)>?\s*$', i.text)
    assert m, i.text
    return m.group(1)


def _walk(ins, labels, start, mask_off, stop):
    """Indices of the instructions executed from `start` on the path with live lanes and a null mask, until stop(ins) holds."""
    path, k, mask_regs, null_means = [], start, None, None
    while k < len(ins):
        i = ins[k]
        path.append(k)
        if stop(i):
            return path
        ld = _kernarg_load(i)
        if ld and ld[0] <= mask_off <= ld[1] - 7:             # the register pair that receives the mask pointer
            first = int(re.match(r'^s_load_\w+\s+s\[?(\d+)', i.text).group(1)) + (mask_off - ld[0]) // 4
            mask_regs = 's[%d:%d]' % (first, first + 1)
        cm = re.match(r'^s_cmp_(eq|lg)_u64\s+(\S+),\s*0$', i.text)
        if cm and cm.group(2) == mask_regs:
            null_means = cm.group(1) == 'eq'                  # the condition that follows is true for a null mask
        if i.op == 's_branch':
            k = labels[_target(i)]
            continue
        if i.op.startswith('s_cbranch_'):
            cond = i.op[len('s_cbranch_'):]
            if cond in ('execz',):
                taken = False                                 # there are live lanes
            elif cond in ('execnz',):
                taken = True
            else:
                assert null_means is not None, 'a branch on something other than the mask on the walked path: ' + i.text
                taken = null_means if cond in ('vccnz', 'scc1') else (not null_means)
                null_means = None
            if taken:
                k = labels[_target(i)]
                continue
        k += 1
    raise AssertionError('walked off the end of the kernel')


def _trips(ins, path):
    """[(index in path of the closing wait, [loads], lines first requested by this trip)] along a path"""
    seen, batch, trips = set(), [], []
    for n, k in enumerate(path):
        i = ins[k]
        ld = _kernarg_load(i)
        if ld:
            batch.append(ld)
        elif i.op == 's_waitcnt' and 'lgkmcnt(0)' in i.text and batch:
            lines = {b // 64 for lo, hi in batch for b in range(lo, hi + 1, 4)}
            trips.append((n, batch, sorted(lines - seen)))
            seen |= lines
            batch = []
    return trips


def test_one_trip_to_the_kernel_arguments_misses_on_the_way_to_the_first_arithmetic(kernel):
    ins, labels, mask_off = kernel
    path = _walk(ins, labels, 0, mask_off, lambda i: bool(ARITH.match(i.text)))
    trips = _trips(ins, path)
    for n, batch, new in trips:
        print('wait at path position %3d: %2d loads, %s' % (n, len(batch), 'new lines ' + ', '.join(hex(64 * x) for x in new)
                                                             if new else 'every line requested before'))
    missing = [t for t in trips if t[2]]
    assert len(trips) >= 1
    assert len(missing) <= 1, 'the parent made 4: %r' % [[hex(64 * x) for x in t[2]] for t in missing]
    # and that one sits in front of the state loads: nothing between them and the arithmetic waits for a line from memory
    first_state_load = next(n for n, k in enumerate(path) if ins[k].op.startswith('global_load'))
    assert all(t[0] < first_state_load for t in missing)
    # the entry block asks for every line of the explicit arguments
    entry_lines = {b // 64 for lo, hi in trips[0][1] for b in range(lo, hi + 1, 4)}
    assert entry_lines >= set(range((mask_off + 8 + 63) // 64)), sorted(entry_lines)
    assert trips[0][0] < next(n for n, k in enumerate(path) if ins[k].op.startswith('s_cbranch'))      # in front of the bounds check


def _loop_exit(ins, labels):
    """Index of the backward branch that closes the sub-step loop: the longest loop of the kernel."""
    best = None
    for k, i in enumerate(ins):
        if i.op.startswith('s_cbranch_') and labels[_target(i)] < k:
            span = k - labels[_target(i)]
            if best is None or span > best[0]:
                best = (span, k)
    assert best and best[0] > 1500, best          # about 2 100 vector instructions per pass
    return best[1]


def test_the_post_step_parameters_arrive_behind_the_kinematics(kernel):
    """The batch of scalar loads at the top of the post-step code (PARAMS_REREAD) is waited for behind the post-step forward
    kinematics: at least 60 vector instructions sit between its last load and its wait."""
    ins, labels, mask_off = kernel
    k0 = _loop_exit(ins, labels) + 1
    path = _walk(ins, labels, k0, mask_off, lambda i: i.op == 's_waitcnt' and 'lgkmcnt(0)' in i.text)
    loads = [n for n, k in enumerate(path) if _kernarg_load(ins[k])]
    assert len(loads) >= 6, loads
    between = sum(ins[k].op.startswith('v_') for k in path[loads[-1] + 1:])
    print('%d scalar loads, %d vector instructions between the last of them and the wait' % (len(loads), between))
    assert between >= 60


def test_census_of_the_headline_kernel_is_unchanged(kernel):
    """4 291 vector instructions, 2 101 of them inside a loop -- one pass of the sub-step loop and of the puck's -- as
    profiles/tools/slot_census.py counts them (profiles/step_spill_traffic.md, section 2): the entry is data movement, no
    vector instruction was added or removed."""
    ins, labels, _ = kernel
    in_loop = set()
    for k, i in enumerate(ins):
        if i.op.startswith('s_cbranch_') and labels[_target(i)] < k:
            in_loop |= set(range(labels[_target(i)], k + 1))
    assert sum(i.op.startswith('v_') for i in ins) == 4291
    assert sum(ins[k].op.startswith('v_') for k in in_loop) == 2101
