"""The communicator of a slab rank: the slice of ``Master`` (src/master_parallel.cxx) and ``Transpose`` that HotPath needs, shaped
after Master_rccl in host/mhh_host_rccl.h. The only module of the package that touches torch.distributed."""
import torch
import torch.distributed as dist


class Master:
    """Decides ONCE how this rank talks to the others:
    local        one rank without MHH_FORCE_COMM: every exchange is a copy
    host_staged  device tensors over gloo (several ranks rehearsing on one card): gloo has no device-side send/recv or all-to-all,
                 so the MESSAGES (never the compute) pass through host copies
    direct       torch.distributed on the tensors as they are: RCCL on the device (the product path) or gloo on CPU tensors"""

    def __init__(self, npy, rank, group, device, force_comm):
        self.npy, self.rank, self.group, self.device, self.force_comm = npy, rank, group, device, force_comm
        self.on_gpu = device.type == "cuda"
        self.mode = ("local" if npy == 1 and not force_comm else
                     "host_staged" if self.on_gpu and dist.is_initialized() and dist.get_backend(group) == "gloo" else "direct")
        self.wire = torch.device("cpu") if self.mode == "host_staged" else device        # where a message's tensors sit
        self.south, self.north = (rank - 1) % npy, (rank + 1) % npy
        self.ranks = dist.get_process_group_ranks(group) if group is not None else list(range(npy))
        self._side, self._slice_events = None, [[]]

    def _on_wire(self, send, recv):
        """send and recv as the messages see them: themselves, or (host-staged) a host copy and an empty host buffer."""
        if self.wire == self.device:
            return send, recv
        return send.to(self.wire), torch.empty_like(recv, device=self.wire)

    def ring(self, send, recv, nn, ns):
        """send = [northbound, nn elements | southbound, ns] -> recv = [what the south neighbour sent north | what the north one sent
        south]: my northbound part arrives as my north neighbour's first part, so with two ranks the whole buffer is ONE message pair."""
        if self.mode == "local":                                 # both neighbours are this rank: a local swap
            recv[:nn].copy_(send[:nn]); recv[nn:nn+ns].copy_(send[nn:nn+ns])
            return
        hs, hr = self._on_wire(send, recv)
        north, south, gr = self.ranks[self.north], self.ranks[self.south], self.group
        if self.north == self.south:
            parts = [(dist.isend, hs, north), (dist.irecv, hr, north)]
        else:                                                    # a part of length 0 is left out
            parts = [(dist.isend, hs[:nn], north), (dist.isend, hs[nn:nn+ns], south), (dist.irecv, hr[:nn], south), (dist.irecv, hr[nn:nn+ns], north)]
        for w in dist.batch_isend_irecv([dist.P2POp(op, t, peer, gr) for op, t, peer in parts if t.numel()]):
            w.wait()
        if hr is not recv:
            recv.copy_(hr)

    def all_to_all(self, send, recv):
        """One equal-split all-to-all (Transpose::exec_xy / exec_yx; RCCL over xGMI)."""
        if self.mode == "local":
            recv.copy_(send)
            return
        hs, hr = self._on_wire(send, recv)
        dist.all_to_all_single(hr, hs, group=self.group)
        if hr is not recv:
            recv.copy_(hr)

    def max(self, value):
        """MAX over ranks of a local maximum (Master::max, src/master_parallel.cxx:233-266)."""
        if self.mode == "local":
            return value
        t = torch.tensor([value], device=self.wire, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=self.group)
        return float(t.item())

    def sum_(self, t):
        """SUM over ranks, element by element; the result sits on this rank's device."""
        if self.mode != "local":
            t = t.to(self.wire)
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)
        return t.to(self.device)

    def barrier(self):
        if self.npy > 1 and dist.is_initialized():
            dist.barrier(self.group)

    def side_stream(self):
        """(second stream, [event, event]) for an exchange that travels beside compute: made on first use, None on the CPU."""
        if self._side is None and self.on_gpu:
            self._side = (torch.cuda.Stream(self.device), [torch.cuda.Event(), torch.cuda.Event()])
        return self._side

    def slice_events(self, n):
        """Four events per k-slice of the pressure solve (ready and done, each way), re-made when the slice count changes."""
        if len(self._slice_events[0]) != n:
            self._slice_events = [[torch.cuda.Event() for _ in range(n)] for _ in range(4)]
        return self._slice_events
