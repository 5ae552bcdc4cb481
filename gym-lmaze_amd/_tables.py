"""The table arguments of the closed-loop rollouts and of evaluate_tables(), each rule written once: "exactly one of",
probs / logits / thresholds -> one checked threshold table, policy / q -> one checked greedy table.  Host side only;
nothing here launches."""
import torch

from . import _abi


def exactly_one(who, **given):
    """`who` wants exactly one of the named arguments; returns the name of the one that is there."""
    there = [n for n, v in given.items() if v is not None]
    if len(there) != 1:
        names = ["%s=" % n for n in given]
        raise ValueError("%s wants exactly one of %s and %s" % (who, ", ".join(names[:-1]), names[-1]))
    return there[0]


def threshold_table(probs, logits, thresholds, temperature, rows, A, device, what, prefix=""):
    """The table a sampling kernel reads: a contiguous, 16-byte aligned uint32 (or int32, the same bits) tensor [rows, W] on
    `device`, W = 4 for A = 4 actions (three thresholds and a reserved word) and A - 1 otherwise -- of exactly one of
    probs       float [rows, A] on `device`: _abi.sampling_thresholds(probs, actions=A);
    logits      float [rows, A] on `device`: sampling_thresholds(softmax(logits.double() / temperature)), temperature > 0;
    thresholds  the table itself, checked and handed back: the caller's memory, never a copy.
    The caller has counted the sources (exactly_one).  prefix ("controller_") and what ("key='ball', G=11") are what the
    refusals call the arguments and say of the table's size."""
    W = 4 if A == 4 else A - 1
    if thresholds is None:
        src, name = (probs, "probs") if logits is None else (logits, "logits")
        if not (isinstance(src, torch.Tensor) and src.is_floating_point() and src.device == device
                and tuple(src.shape) == (rows, A)):
            raise ValueError("%s%s must be a float tensor [%d, %d] on %s (%s)" % (prefix, name, rows, A, device, what))
        if logits is not None:
            if not float(temperature) > 0.0:
                raise ValueError("temperature must be > 0")
            src = torch.softmax(logits.double() / float(temperature), -1)
        thresholds = _abi.sampling_thresholds(src, actions=A)
    if not (isinstance(thresholds, torch.Tensor) and thresholds.dtype in (torch.uint32, torch.int32)
            and thresholds.device == device and thresholds.is_contiguous() and tuple(thresholds.shape) == (rows, W)
            and thresholds.data_ptr() % 16 == 0):
        raise ValueError("%sthresholds must be a contiguous, 16-byte aligned uint32 tensor [%d, %d] on %s (%s)"
                         % (prefix, rows, W, device, what))
    return thresholds


def greedy_table(q):
    """The greedy action table uint8[S] of a float tensor q[S, A] (A <= 255), on q's device: the FIRST maximum of every
    row, spelled out (the lowest index whose value equals the row's maximum) and not left to argmax's tie behaviour.
    A row that holds a NaN equals its maximum nowhere and gets the id A, which every step treats as no move."""
    if not (isinstance(q, torch.Tensor) and q.dim() == 2 and q.is_floating_point() and 1 <= q.shape[1] <= 255):
        raise ValueError("q must be a float tensor [S, A] with 1 <= A <= 255")
    A = q.shape[1]
    idx = torch.arange(A, device=q.device, dtype=torch.int32).expand_as(q)
    first = torch.where(q == q.max(dim=1, keepdim=True).values, idx, torch.full_like(idx, A)).min(dim=1).values
    return first.to(torch.uint8)


def greedy_policy(policy, q, entries, device, what):
    """rollout_policy()'s table: policy itself, or greedy_table(q), as a contiguous uint8 tensor of `entries` entries on
    `device`.  what: what the refusal says of the table's size."""
    if q is not None:
        if not isinstance(q, torch.Tensor) or q.device != device:
            raise ValueError("q must be a float tensor [S, A] on %s" % device)
        policy = greedy_table(q)
    if not (isinstance(policy, torch.Tensor) and policy.dtype == torch.uint8 and policy.device == device
            and policy.is_contiguous() and policy.numel() == entries):
        raise ValueError("policy must be a contiguous uint8 tensor of %d entries on %s (%s)" % (entries, device, what))
    return policy
