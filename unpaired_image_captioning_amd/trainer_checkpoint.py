"""Checkpoints of the Trainer (trainer.py; DESIGN.md, "Checkpoints"): the asynchronous snapshot, the writer thread, and the load
that continues a run bit for bit.  One Checkpointer per Trainer: it reads and, on load, writes the Trainer it was built for --
models, arenas, counters, exchange and opt are looked up when a save or load runs, never cached (a benchmark swaps
`trainer.exchange`, a caller redirects `opt.checkpoint_path`)."""
import os
import threading
import warnings

import numpy as np
import torch

STATE_VERSION = 1


def write(obj, path):
    """torch.save to a temporary name, then os.replace: a reader never sees half a file."""
    tmp = path + '.tmp'
    torch.save(obj, tmp)
    os.replace(tmp, path)


def _read(path, names):
    """The first of `names` that exists under `path`, loaded as data only (weights_only), else None."""
    for name in names:
        f = os.path.join(path, name)
        if os.path.isfile(f):
            return torch.load(f, map_location='cpu', weights_only=True)
    return None


class Snapshot(object):
    """What one model contributes to a checkpoint, copied twice: device-to-device on the step's stream into `dev` (the step
    goes on and changes the arena), from there to the pinned `host` buffers on the copy stream.  Rows of dev / host: the
    arena's flat and its state arenas (FlatArena.states: two for Adam, none for sgd) up to the scalar slots.  `extra`:
    state_dict entries that do not live in the arena -- the BatchNorm buffers -- as {key: [device copy, pinned copy]}.  All buffers are allocated once and reused by every save."""

    def __init__(self, arena):
        self.n = arena.scalars_off if arena is not None else 0
        self.rows = 1 + len(arena.states) if arena is not None else 0
        self.dev = self.host = None
        if arena is not None:
            self.dev = torch.empty(self.rows, self.n, dtype=torch.float32, device=arena.flat.device)
            # (one host tensor per row: torch.save writes a view's WHOLE storage, and the weights and the moments go to two files)
            self.host = [torch.empty(self.n, dtype=torch.float32, pin_memory=arena.flat.is_cuda) for _ in range(self.rows)]
        self.extra = {}
        self.layout = []

    def take(self, model, arena):
        """On the current stream: arena -> dev, and the layout of model.state_dict(): (key, arena offset or None, shape)."""
        if arena is not None:
            for row, src in enumerate([arena.flat] + arena.states):
                self.dev[row].copy_(src[:self.n])
        self.layout = []
        for k, v in model.state_dict().items():
            v = v.detach()
            off = arena.offsets.get(k) if arena is not None else None
            if off is not None and v.data_ptr() != arena.flat.data_ptr() + 4 * off:
                off = None                                  # (a parameter that was re-homed after the arena was built)
            if off is None:
                slot = self.extra.get(k)
                if slot is None or slot[0].shape != v.shape or slot[0].dtype != v.dtype or slot[0].device != v.device:
                    slot = self.extra[k] = [torch.empty_like(v), torch.empty(v.shape, dtype=v.dtype, pin_memory=v.is_cuda)]
                slot[0].copy_(v)
            self.layout.append((k, off, tuple(v.shape)))

    def to_host(self):
        """On the copy stream, behind the event that follows take()."""
        if self.dev is not None:
            for row in range(self.rows):
                self.host[row].copy_(self.dev[row], non_blocking=True)
        for k, off, _ in self.layout:
            if off is None:
                self.extra[k][1].copy_(self.extra[k][0], non_blocking=True)

    def state_dict(self):
        """The model's state_dict as views of the pinned buffers (once the copy stream's event has completed)."""
        out = {}
        for k, off, shape in self.layout:
            n = int(np.prod(shape, dtype=np.int64))
            out[k] = self.host[0][off:off + n].view(shape) if off is not None else self.extra[k][1]
        return out


class Checkpointer(object):
    """State, all of it owned here: `_snapshots` ({model kind: Snapshot}, allocated by the first save), `_copy_stream` (the
    snapshots' device-to-host copies; created by the first save of device models -- the prefetch copies on a stream of its own,
    trainer_ship.py: each role only ever waits on its own events, so one stream never ordered the two), `_save_thread` with
    its error slot `_save_error`."""

    def __init__(self, trainer):
        self.trainer = trainer
        self._snapshots = {}
        self._copy_stream = None
        self._save_thread = None
        self._save_error = None

    def _seed_counters_begin(self):
        """The models' _seed_counter of every rank, collected with ONE small collective: every rank writes the 16-bit halves of
        its counters (exact as floats) into its own slots of a zero vector, and the vector is summed on the current stream.
        Returns (model kinds, rows): rows is a host list on one rank, else a HOST tensor [world, 2 * kinds] -- for device models a
        pinned one that an asynchronous copy on the CURRENT stream fills, right behind the sum: the device tensor is allocated,
        summed and read on one stream, so the allocator may hand its block on as soon as this returns.  Nobody waits here;
        _seed_counters_end reads the rows once an event recorded behind this call has completed."""
        tr = self.trainer
        ex = tr.exchange
        world, rank = ex.world_size, ex.rank
        mods = [('i2t', tr.i2t_model), ('nmt', tr.nmt_model)]
        mods = [(k, m) for k, m in mods if m is not None and hasattr(m, '_seed_counter')]
        mine = [h for _, m in mods for h in (int(m._seed_counter) >> 16, int(m._seed_counter) & 0xFFFF)]
        kinds = [k for k, _ in mods]
        if world == 1 or not mods:
            return kinds, [mine]
        t = torch.zeros(world, len(mine), dtype=torch.float32)
        t[rank] = torch.tensor(mine, dtype=torch.float32)
        dev = next(mods[0][1].parameters()).device
        if dev.type != 'cuda':
            ex._sum(t)
            return kinds, t
        with torch.cuda.device(dev):
            t = t.pin_memory().to(dev, non_blocking=True)
            ex._sum(t)
            rows = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
            rows.copy_(t, non_blocking=True)
        return kinds, rows

    @staticmethod
    def _seed_counters_end(kinds, rows):
        if torch.is_tensor(rows):
            rows = [[int(x) for x in row] for row in rows.tolist()]
        return {k: [(row[2 * j] << 16) | row[2 * j + 1] for row in rows] for j, k in enumerate(kinds)}

    def save_async(self, tag=''):
        """save_models without the wait: the step's stream only copies the arenas device-to-device into a snapshot (behind the
        step's Adam, and behind the gathers of the sharded exchange); the snapshot travels to pinned host memory on the copy
        stream and a writer thread writes the files from there, while the following steps run.  Counters and seed counters are
        taken now, on the host.  A save still in flight is waited for first; wait() joins the writer and re-raises
        what it failed with.  The device-to-device copy stays on the step's stream on purpose: a kernel on a side stream beside
        a persistent recurrence launch is what Trainer._finish_step names as a cause of PersistentTimeout."""
        self.wait()
        tr = self.trainer
        path = tr.opt.checkpoint_path
        ex = tr.exchange
        writer = ex is None or ex.rank == 0
        nmt = tr.nmt_model is not None and bool(getattr(tr.opt, 'nmt_train_flag', 0))
        if tr.arena is not None and tr.sharded:
            dev = tr.arena.flat.device        # (the pipelined piece's Adam and the weights' all-gathers run on the communication stream)
            torch.cuda.current_stream(dev).wait_stream(tr._comm(dev))
        tr.gather_masters()          # (sharded bf16 exchange: a collective -- every rank calls save_models, as every rank runs the loop)
        if tr.arena is not None:
            tr.arena.gather_moments(ex)
        if nmt:
            tr.optim.nmt_arena.gather_moments(tr.optim.exchange)
        kinds, rows = self._seed_counters_begin()
        o = tr.optim if nmt else None
        on_gpu = torch.is_tensor(rows) and rows.is_pinned()
        state = {'format_version': STATE_VERSION, 'world_size': ex.world_size, 'step': tr._step,
                 'i2t_current_lr': float(tr.i2t_current_lr), 'sc_flag': bool(tr.sc_flag),
                 'ss_prob': float(getattr(tr.i2t_model, 'ss_prob', 0.0)) if tr.i2t_model is not None else 0.0,
                 'optim': None if o is None else o.counters()}
        # (optional keys: a file without them was written when every arena ran Adam)
        if tr.arena is not None:
            state['i2t_optim'] = tr.arena.method
        if nmt:
            state['nmt_optim'] = o.nmt_arena.method
        if not writer:
            return                   # one writer: the ranks hold identical weights
        # (kind, model, arena, the optimizer's lr / betas / eps / step / weight decay for the optimizer file)
        jobs = []
        if tr.i2t_model is not None:
            jobs.append(('i2t', tr.i2t_model, tr.arena, (tr.i2t_current_lr, tr.betas, tr.eps, tr._step, tr.weight_decay)))
        if nmt:
            jobs.append(('nmt', tr.nmt_model, o.nmt_arena, (o.nmt_current_lr, (o.nmt_optim_alpha, o.nmt_optim_beta), o.nmt_optim_epsilon,
                                                           o._nmt_steps, o.nmt_weight_decay)))
        snaps = self._snapshots
        with torch.no_grad():
            for kind, model, arena, _ in jobs:
                snap = snaps.get(kind)
                if snap is None or snap.n != (arena.scalars_off if arena is not None else 0):
                    snap = snaps[kind] = Snapshot(arena)
                snap.take(model, arena)
                on_gpu = on_gpu or any(p.is_cuda for p in model.parameters())
        done = None
        if on_gpu:
            ready = torch.cuda.Event()
            ready.record()
            if self._copy_stream is None:
                self._copy_stream = torch.cuda.Stream()
            with torch.cuda.stream(self._copy_stream), torch.no_grad():
                self._copy_stream.wait_event(ready)
                for kind, _, _, _ in jobs:
                    snaps[kind].to_host()
                done = torch.cuda.Event()
                done.record()
        else:
            for kind, _, _, _ in jobs:
                snaps[kind].to_host()
        files = [(kind, arena, snaps[kind], adam) for kind, _, arena, adam in jobs]
        self._save_error = None
        self._save_thread = threading.Thread(target=self._write_checkpoint, args=(path, tag, done, files, state, kinds, rows))
        self._save_thread.start()

    def _write_checkpoint(self, path, tag, done, files, state, kinds, rows):
        """The writer thread: waits for the copy stream's event, then writes every file from the pinned buffers."""
        try:
            if done is not None:
                done.synchronize()
            os.makedirs(path, exist_ok=True)
            for kind, arena, snap, (lr, betas, eps, step, wd) in files:
                write(snap.state_dict(), os.path.join(path, 'model_%s%s.pth' % (kind, tag)))
                if arena is not None:
                    write(arena.optimizer_state_from(snap.host[1:], lr, betas, eps, step, wd),
                          os.path.join(path, 'optimizer_%s%s.pth' % (kind, tag)))
            state['seed_counters'] = self._seed_counters_end(kinds, rows)
            write(state, os.path.join(path, 'trainer_state' + tag + '.pth'))
        except Exception as e:              # (handed to wait)
            self._save_error = e

    def wait(self):
        """Join the writer thread of the save in flight, if any, and re-raise what it failed with."""
        t = self._save_thread
        if t is None:
            return
        t.join()
        self._save_thread = None
        err, self._save_error = self._save_error, None
        if err is not None:
            raise err

    def load(self, path=None, tag='-best'):
        """Continue from what save_models(tag) wrote under `path` (default: opt.start_from, P/opts.py:37): the weights with the
        BatchNorm buffers, the Adam state -- under the name save_models writes, optimizer_i2t{tag}.pth, or the one the reference
        loads, i2t_optimizer.pth (P/misc/optimizer.py:80-87) -- and trainer_state.  The pivot NMT half is loaded when build_nmt
        has run.  A missing optimizer or trainer_state file means weights only and a fresh optimizer, as in the reference, with a
        warning; an unknown trainer_state version raises.  A file written at another world size loads: rank r takes the r-th seed
        counter when there is one, else the first with its rank mixed in (trainer.rank_seed).  The carried next-batch
        denominator, a prefetched batch and the gather events are not part of a checkpoint: they are reset."""
        from .trainer import rank_seed
        self.wait()                              # (a save in flight reads the snapshot, not the arenas, but may be writing these files)
        tr = self.trainer
        path = getattr(tr.opt, 'start_from', None) if path is None else path
        if path is None:
            raise ValueError("load_models: no path given and opt.start_from is not set")
        state = _read(path, ['trainer_state' + tag + '.pth'])
        if state is not None and state.get('format_version') != STATE_VERSION:
            raise ValueError("trainer_state%s.pth has format version %r, this library reads version %d"
                             % (tag, state.get('format_version'), STATE_VERSION))
        if state is None:
            warnings.warn("load_models: no trainer_state%s.pth under %s -- counters and seeds start afresh" % (tag, path))
        if state is not None:
            # before anything is written: a checkpoint of another --i2t_optim / --nmt_optim does not continue under this one
            # (for the models whose files are there; a state without the key was written when every arena ran Adam)
            for kind, method in (('i2t', tr.method if tr.i2t_model is not None else None),
                                 ('nmt', tr.optim.nmt_method if tr.nmt_model is not None else None)):
                theirs = state.get(kind + '_optim', 'adam')
                if method is not None and theirs != method and os.path.isfile(os.path.join(path, 'model_%s%s.pth' % (kind, tag))):
                    raise ValueError("trainer_state%s.pth was written with %s_optim='%s', this run is configured with '%s'"
                                     % (tag, kind, theirs, method))
        seeds = state['seed_counters'] if state is not None else {}
        rank = tr.exchange.rank

        def seed_for(kind, model):
            c = seeds.get(kind)
            if c:
                model._seed_counter = int(c[rank]) if rank < len(c) else rank_seed(int(c[0]), rank)

        loaded = False
        sd = _read(path, ['model_i2t' + tag + '.pth']) if tr.i2t_model is not None else None
        if sd is not None:
            loaded = True
            if tr.arena is None:
                tr.build_optimizer()
            a = tr.arena
            if tr.sharded:
                dev = a.flat.device              # (all-gathers of an earlier step may still be writing the operand copy)
                torch.cuda.current_stream(dev).wait_stream(tr._comm(dev))
            tr.i2t_model.load_state_dict(sd)     # (in place: every parameter is its view of the arena)
            osd = _read(path, ['optimizer_i2t' + tag + '.pth', 'i2t_optimizer.pth'])
            if osd is not None:
                tr._step, tr.i2t_current_lr = a.import_optimizer_state(osd)
            else:
                warnings.warn("load_models: no optimizer_i2t%s.pth / i2t_optimizer.pth under %s -- weights only, fresh %s"
                              % (tag, path, 'Adam' if a.method == 'adam' else a.method))
                for buf in a.states:
                    buf.zero_()
                a.sync_operand_copy()
                a.masters_stale = False
                tr._step, tr.i2t_current_lr = 0, tr.lr
            if state is not None:
                tr.i2t_model.ss_prob = state['ss_prob']
                tr.sc_flag = state['sc_flag']
                if osd is not None:
                    tr._step, tr.i2t_current_lr = state['step'], state['i2t_current_lr']
                seed_for('i2t', tr.i2t_model)
            tr._reset_step_carry()
        sd = _read(path, ['model_nmt' + tag + '.pth']) if tr.nmt_model is not None else None
        if sd is not None:
            loaded = True
            tr.nmt_model.load_state_dict(sd)
            osd = _read(path, ['optimizer_nmt' + tag + '.pth', 'nmt_optimizer.pth'])
            if osd is not None and not isinstance(osd, dict):
                raise ValueError("the NMT optimizer file under %s is not a state dict" % path)
            counters = dict(state['optim']) if (state is not None and state.get('optim') and osd is not None) else {}
            if osd is None:
                n = tr.optim.nmt_arena
                warnings.warn("load_models: no optimizer_nmt%s.pth / nmt_optimizer.pth under %s -- weights only, fresh %s"
                              % (tag, path, 'Adam' if n.method == 'adam' else n.method))
                for buf in n.states:
                    buf.zero_()
                tr.optim._step = tr.optim._nmt_steps = 0
                tr.optim.nmt_current_lr = tr.optim.nmt_lr
            else:
                tr.optim.load_state_dict(dict(counters, nmt=osd))
            if state is not None:
                seed_for('nmt', tr.nmt_model)
        if not loaded:
            raise FileNotFoundError("load_models: neither model_i2t%s.pth nor model_nmt%s.pth for the models built here under %s"
                                    % (tag, tag, path))
