"""Count the spill-traffic instructions in the step-loop copies of a ppo_update_kernel
instantiation, from the gfx950 assembly of ppo_update.hip (no GPU):

  hipcc <the library's flags> --cuda-device-only -S -Rpass-analysis=kernel-resource-usage \
      xagents_amd/csrc/ppo_update.hip -o ppo_update.s
  python tools/ppo_loop_counts.py ppo_update.s [mangled-name substring]

The step loops are the strongly connected components of the kernel's block graph with more
than 1500 instructions (the code that can run again within a launch: blocks that only leave,
such as a poll's time-out exit, are outside); each is labelled by the hand-off stores it holds
(plain / sc1 / both). For each: the static count of every class and the part of it on blocks
that only a poll's slow path runs (those with its sleep, the wall clock or the abort word)."""
import re
import sys
from collections import Counter

HEAD = 'ppo_update_kernelILi4ELi2ELi16ELb0ELb1ELi3E'
CLASSES = ['v_readlane', 'v_readfirstlane', 'v_writelane', 'v_accvgpr', 's_nop', 's_waitcnt',
           's_load', 's_cbranch', 'v_cmp', 'buffer_store', 'buffer_load', 's_barrier', 'ds_',
           'v_cndmask']
DPP = '*_dpp'  # any VALU instruction with a DPP operand (counted by its mnemonic's suffix)


def kernel_body(path, name):
    lines, on = [], False
    for ln in open(path):
        if not on:
            if re.match(r'^_Z\S*%s\S*:' % re.escape(name), ln):
                on = True
            continue
        if ln.startswith('\t.end_amdhsa_kernel') or ln.startswith('.Lfunc_end'):
            break
        lines.append(ln.rstrip('\n'))
    return lines


def parse(lines):
    """[(label or None, mnemonic, text)] for instruction lines, labels attached to the next."""
    out, pending = [], []
    for ln in lines:
        s = ln.split(';')[0].rstrip()
        m = re.match(r'^(\.LBB\d+_\d+):', s)
        if m:
            pending.append(m.group(1))
            continue
        s = s.strip()
        if not s or s.startswith('.') or s.endswith(':'):
            continue
        out.append((tuple(pending), s.split()[0], s))
        pending = []
    return out


def blocks(ins):
    """Basic blocks [(first, last)] and their successor lists (by block number)."""
    lead = {0}
    pos = {}
    for i, (labs, mn, _) in enumerate(ins):
        for l in labs:
            pos[l] = i
        if labs:
            lead.add(i)
        if (mn.startswith('s_cbranch') or mn in ('s_branch', 's_endpgm', 's_setpc_b64')) and \
                i + 1 < len(ins):
            lead.add(i + 1)
    first = sorted(lead)
    bl = [(a, (first[n + 1] if n + 1 < len(first) else len(ins)) - 1) for n, a in enumerate(first)]
    at = {a: n for n, (a, _) in enumerate(bl)}
    succ = []
    for n, (a, b) in enumerate(bl):
        mn, txt = ins[b][1], ins[b][2]
        s = []
        if mn.startswith('s_cbranch') or mn == 's_branch':
            t = txt.split()[-1]
            if t in pos:
                s.append(at[pos[t]])
        if mn not in ('s_branch', 's_endpgm', 's_setpc_b64') and n + 1 < len(bl):
            s.append(n + 1)
        succ.append(s)
    return bl, succ


def sccs(succ):
    """Strongly connected components of the block graph (Tarjan, iterative), each a set."""
    n, idx, low, on, st, out, c = len(succ), {}, {}, set(), [], [], 0
    for r in range(n):
        if r in idx:
            continue
        work = [(r, 0)]
        while work:
            v, i = work.pop()
            if i == 0:
                idx[v] = low[v] = c
                c += 1
                st.append(v)
                on.add(v)
            if i < len(succ[v]):
                work.append((v, i + 1))
                u = succ[v][i]
                if u not in idx:
                    work.append((u, 0))
                elif u in on:
                    low[v] = min(low[v], idx[u])
                continue
            if low[v] == idx[v]:
                comp = set()
                while True:
                    u = st.pop()
                    on.discard(u)
                    comp.add(u)
                    if u == v:
                        break
                out.append(comp)
            if work:
                low[work[-1][0]] = min(low[work[-1][0]], low[v])
    return out


def count(ins, bl, body):
    c = Counter()
    for n in body:
        for i in range(bl[n][0], bl[n][1] + 1):
            mn = ins[i][1]
            for k in CLASSES:
                if mn.startswith(k):
                    c[k] += 1
            if mn.endswith('_dpp'):
                c[DPP] += 1
            c['instructions'] += 1
    return c


SLOW = ('s_sleep', 's_memrealtime', 's_endpgm')


def main(path, name=HEAD):
    ins = parse(kernel_body(path, name))
    if not ins:
        sys.exit(f'no kernel matching {name} in {path}')
    bl, succ = blocks(ins)
    step = [c for c in sccs(succ) if sum(bl[n][1] - bl[n][0] + 1 for n in c) > 1500]
    print(f'{name}: {len(ins)} instructions, {len(step)} step-loop copies')
    for body in sorted(step, key=min):
        st = [ins[i][2] for n in body for i in range(bl[n][0], bl[n][1] + 1)
              if ins[i][1].startswith('buffer_store')]
        sc1 = sum(' sc1' in t for t in st)
        kind = 'plain (form 2)' if sc1 == 0 else 'write-through (form 1)' if sc1 == len(st) \
            else 'general (form 0)'
        # a poll's slow path: the blocks holding its sleep, the wall clock or the abort /
        # status word accesses (global_load / global_store)
        slow = {n for n in body if any(
            ins[i][1] in SLOW or ins[i][1].startswith('global_')
            for i in range(bl[n][0], bl[n][1] + 1))}
        tot, slw = count(ins, bl, body), count(ins, bl, slow)
        print(f'\n  {kind}: {len(body)} blocks, {len(slow)} of them on poll slow paths')
        print(f'    {"class":<18}{"static":>8}{"slow-path blocks":>18}')
        for k in ['instructions'] + CLASSES + [DPP]:
            print(f'    {k:<18}{tot[k]:>8}{slw[k]:>18}')


if __name__ == '__main__':
    main(*sys.argv[1:])
