"""On-device training samplers.

DeviceWarpSampler (SAS): the reference's ``WarpSampler`` (BS/dataloaders/sas.py:93-122) with the
per-sequence work of ``sample_function`` (:65-91) done by one HIP kernel (rs_sas_sample).

Same contract as the reference loader: iterate ``len(sampler) = len(user_train) // batch_size`` batches
of (seq, pos, neg), each (batch_size, max_len); a row is a uniformly drawn user's last ``max_len``
items shifted by one (seq/pos), left-padded with 0, and negatives drawn uniformly from
{0..item_num} minus that window (item 0 is a legal negative, as ``random_neq`` allows).  Unlike the
reference the batch is produced on the device (int64 tensors) by a counter-based RNG: no worker
processes, no host round trip, and ``sample_into`` can be captured in the training step's HIP graph.

DeviceBertMasker (BERT4Rec): the reference's ``BertTrainDataset`` + shuffling ``DataLoader``
(BS/dataloaders/bert.py:64-110) with the per-token cloze masking done by rs_bert_mask.  An epoch visits
the users in a fresh random order (``torch.randperm`` on the device at ``__iter__``), ``len(masker) =
n_users // batch_size`` full batches (the fixed batch shape a captured graph needs; the reference's
last partial batch is dropped), each row = that user's last ``max_len`` items cloze-masked at
``mask_prob`` (80 % [MASK] = num_items+1, 10 % random item, 10 % kept), labels = the masked items.
"""
import torch

from . import ops


def _flatten(histories, device):
    lens = [len(s) for s in histories]
    if not lens or min(lens) < 1:
        raise ValueError("every user needs at least one training item")
    off = torch.zeros(len(lens) + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(torch.tensor(lens, dtype=torch.int64), 0)
    items = torch.tensor([i for s in histories for i in s], dtype=torch.int64, device=device)
    return off.to(device), items, len(lens)


class DeviceWarpSampler:
    n_outputs = 3

    def __init__(self, user_train, item_num, batch_size, max_len, device="cuda", num_workers=None, seed=None,
                 shared_negs=None):
        """user_train: list (per user) of item-id lists, as ``data_partition`` builds it.
        num_workers is accepted for signature compatibility and ignored.
        shared_negs=K: batches are (seq, pos, cand) with cand int64 (K,) drawn uniformly with replacement from
        [1, item_num] on the device (rs_uniform_items: the same advanced step seed, its own salt) -- the candidates
        of the sampled-softmax loss, shared by the whole batch; the per-position neg goes to a private buffer."""
        if max_len > 512:
            raise ValueError("max_len must be <= 512")
        self.device = torch.device(device)
        self.offsets, self.items, self.n_users = _flatten(user_train, self.device)
        self.item_num = int(item_num)
        self.batch_size = int(batch_size)
        self.max_len = int(max_len)
        self.num_batch = self.n_users // self.batch_size
        g = torch.Generator().manual_seed(seed) if seed is not None else None
        self.salt = int(torch.randint(0, 2 ** 62, (1,), generator=g).item())
        self.seed_base = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.cnt = 0
        self.shared_negs = None if shared_negs is None else int(shared_negs)
        if self.shared_negs is not None:
            if self.shared_negs < 1:
                raise ValueError("shared_negs must be a positive number of candidates")
            self.cand_salt = int(torch.randint(0, 2 ** 62, (1,), generator=g).item())
            self._neg = torch.empty((self.batch_size, self.max_len), dtype=torch.int64, device=self.device)

    def sample_into(self, seq, pos, neg, draws=None):
        """Write the next batch into existing (batch_size, max_len) int64 device tensors (draws: see
        ops.sas_sample).  With shared_negs=K the third tensor is cand, int64 (K,)."""
        if self.shared_negs is not None:
            cand = neg
            if cand.shape != (self.shared_negs,) or cand.dtype != torch.int64 or not cand.is_contiguous():
                raise ValueError(f"cand must be a contiguous int64 tensor of shape ({self.shared_negs},)")
            ops.sas_sample(self.offsets, self.items, self.n_users, self.item_num, self.seed_base, self.salt, seq, pos,
                           self._neg, draws)
            ops.uniform_items(self.seed_base, self.cand_salt, self.item_num, cand)   # the seed the launch above advanced
            return
        ops.sas_sample(self.offsets, self.items, self.n_users, self.item_num, self.seed_base, self.salt, seq, pos, neg,
                       draws)

    def sample(self):
        shape = (self.batch_size, self.max_len)
        if self.shared_negs is not None:
            seq, pos = (torch.empty(shape, dtype=torch.int64, device=self.device) for _ in range(2))
            cand = torch.empty(self.shared_negs, dtype=torch.int64, device=self.device)
            self.sample_into(seq, pos, cand)
            return seq, pos, cand
        seq, pos, neg = (torch.empty(shape, dtype=torch.int64, device=self.device) for _ in range(3))
        self.sample_into(seq, pos, neg)
        return seq, pos, neg

    # ---- the reference loader's iterator protocol (BS/dataloaders/sas.py:111-122)
    def __iter__(self):
        self.cnt = 0
        return self

    def __next__(self):
        if self.cnt < self.num_batch:
            self.cnt += 1
            return self.sample()
        raise StopIteration

    def __len__(self):
        return self.num_batch

    def close(self):
        pass


class DeviceBertMasker:
    n_outputs = 2

    def __init__(self, u2seq, num_items, batch_size, max_len, mask_prob, device="cuda", seed=None, shared_negs=None):
        """u2seq: list (per user) of training item-id lists (the reference's ``train`` dict values in user
        order).  The [MASK] token is num_items + 1, as BERTEmbedding's table (V+2 rows) expects.
        shared_negs=K: batches are (tokens, labels, cand) with cand int64 (K,) drawn uniformly with replacement from
        [1, num_items] on the device (rs_uniform_items on the step seed rs_bert_mask advanced, its own salt) -- the
        candidates of the sampled-softmax loss, shared by the whole batch."""
        self.shared_negs = None if shared_negs is None else int(shared_negs)
        if self.shared_negs is not None and self.shared_negs < 1:
            raise ValueError("shared_negs must be a positive number of candidates")
        self.n_outputs = 2 if self.shared_negs is None else 3
        self.device = torch.device(device)
        self.offsets, self.items, self.n_users = _flatten(u2seq, self.device)
        self.num_items = int(num_items)
        self.batch_size = int(batch_size)
        self.max_len = int(max_len)
        self.mask_prob = float(mask_prob)
        self.num_batch = self.n_users // self.batch_size
        self.gen = torch.Generator(device=self.device)
        g = torch.Generator()
        if seed is not None:
            g.manual_seed(seed)
            self.gen.manual_seed(seed)
        self.salt = int(torch.randint(0, 2 ** 62, (1,), generator=g).item())
        if self.shared_negs is not None:
            self.cand_salt = int(torch.randint(0, 2 ** 62, (1,), generator=g).item())
        self.state = torch.zeros(2, dtype=torch.int64, device=self.device)   # {step seed, cursor}
        self.perm = torch.arange(self.n_users, dtype=torch.int64, device=self.device)
        self.cnt = 0

    def new_epoch(self):
        """Reshuffle the user order in place and restart the cursor (device work; graphs see it)."""
        torch.randperm(self.n_users, generator=self.gen, device=self.device, out=self.perm)
        self.state[1:2].zero_()

    def sample_into(self, tokens, labels, *rest, draws=None):
        """Write the next batch into existing (batch_size, max_len) int64 device tensors (draws, also accepted as the
        last positional argument: see ops.bert_mask).  With shared_negs=K the third tensor is cand, int64 (K,)."""
        cand = None
        if self.shared_negs is not None:
            if not rest:
                raise ValueError(f"shared_negs={self.shared_negs}: sample_into needs cand")
            cand, rest = rest[0], rest[1:]
            if cand.shape != (self.shared_negs,) or cand.dtype != torch.int64 or not cand.is_contiguous():
                raise ValueError(f"cand must be a contiguous int64 tensor of shape ({self.shared_negs},)")
        if len(rest) > 1 or (rest and draws is not None):
            raise TypeError("sample_into takes (tokens, labels[, cand][, draws])")
        draws = rest[0] if rest else draws
        ops.bert_mask(self.offsets, self.items, self.n_users, self.num_items, self.mask_prob, self.perm, self.state,
                      self.salt, tokens, labels, draws)
        if cand is not None:
            ops.uniform_items(self.state[0:1], self.cand_salt, self.num_items, cand)   # the seed just advanced

    def sample(self):
        shape = (self.batch_size, self.max_len)
        tokens, labels = (torch.empty(shape, dtype=torch.int64, device=self.device) for _ in range(2))
        if self.shared_negs is not None:
            cand = torch.empty(self.shared_negs, dtype=torch.int64, device=self.device)
            self.sample_into(tokens, labels, cand)
            return tokens, labels, cand
        self.sample_into(tokens, labels)
        return tokens, labels

    def __iter__(self):
        self.new_epoch()
        self.cnt = 0
        return self

    def __next__(self):
        if self.cnt < self.num_batch:
            self.cnt += 1
            return self.sample()
        raise StopIteration

    def __len__(self):
        return self.num_batch
