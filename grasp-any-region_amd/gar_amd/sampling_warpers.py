"""``generate(sampling_warpers=...)``: the four sampling warpers of HF's list behind temperature / top-k / top-p — ``min_p``,
``typical_p``, ``epsilon_cutoff``, ``eta_cutoff`` — checked on the host and packed into the four floats ``gar_sample_ext`` reads on
the device (include/gar_hip.h). Pure Python: importing it needs neither torch nor the library.

Semantics are those of transformers' ``MinPLogitsWarper`` -> ``TypicalLogitsWarper`` -> ``EpsilonLogitsWarper`` ->
``EtaLogitsWarper`` in the order ``GenerationMixin._get_logits_processor`` appends them, each with ``min_tokens_to_keep = 1`` and each
over the tokens the stage before it left.
"""
from __future__ import annotations

from dataclasses import dataclass, fields
from typing import List, Optional


def _is_number(v) -> bool:
    return isinstance(v, (int, float)) and not isinstance(v, bool)


@dataclass(frozen=True)
class SamplingWarpers:
    """The further sampling warpers of one ``generate(do_sample=True)`` request, applied on the device after temperature, top-k and
    top-p and before the draw. Every probability below is the softmax over the tokens the previous stage left.

    ``min_p`` in [0, 1] (None or 0 = off): tokens with p < min_p x (the largest p) are removed.
    ``typical_p`` in (0, 1) (None or >= 1 = off): with H the entropy, tokens are ranked by ``|-log p - H|`` and the smallest ones
    are kept until they hold typical_p of the mass (a token stays iff the tokens ranked strictly before it hold less). This stage
    may remove the most likely token.
    ``epsilon_cutoff`` in (0, 1) (None or 0 = off): tokens with p < epsilon are removed, the most likely one always stays.
    ``eta_cutoff`` in (0, 1) (None or 0 = off): the same with ``min(eta, sqrt(eta) * exp(-H))``.

    A value outside its range is a ``ValueError`` — also where HF would silently build no warper for it."""
    min_p: Optional[float] = None
    typical_p: Optional[float] = None
    epsilon_cutoff: Optional[float] = None
    eta_cutoff: Optional[float] = None

    def __post_init__(self):
        set_ = object.__setattr__
        v = self.min_p
        if v is not None:
            # HF MinPLogitsWarper: `min_p` has to be a float in the [0, 1] interval
            if not _is_number(v) or not 0 <= float(v) <= 1.0:
                raise ValueError(f"`min_p` has to be a float in the [0, 1] interval, but is {v!r}")
            set_(self, "min_p", float(v))
        v = self.typical_p
        if v is not None:
            # HF TypicalLogitsWarper: `typical_p` has to be a float > 0 and < 1 (GenerationMixin builds no warper for >= 1)
            if not _is_number(v) or not float(v) > 0:
                raise ValueError(f"`typical_p` has to be a float > 0 (and acts below 1), but is {v!r}")
            set_(self, "typical_p", float(v))
        for name in ("epsilon_cutoff", "eta_cutoff"):
            v = getattr(self, name)
            if v is not None:
                # HF Epsilon / EtaLogitsWarper: a float > 0 and < 1; 0 is GenerationConfig's "off"
                if not _is_number(v) or not 0 <= float(v) < 1.0:
                    raise ValueError(f"`{name}` has to be a float > 0 and < 1 (0 = off), but is {v!r}")
                set_(self, name, float(v))

    @classmethod
    def coerce(cls, value) -> "SamplingWarpers":
        """``generate(sampling_warpers=value)``: None, a SamplingWarpers, or a dict with its field names"""
        if value is None:
            return cls()
        if isinstance(value, cls):
            return value
        if isinstance(value, dict):
            unknown = sorted(set(value) - {f.name for f in fields(cls)})
            if unknown:
                raise TypeError(f"sampling_warpers: unknown keys {unknown} (fields: {[f.name for f in fields(cls)]})")
            return cls(**value)
        raise TypeError(f"sampling_warpers: a SamplingWarpers, a dict or None, not {type(value).__name__}")

    @property
    def neutral(self) -> bool:
        """no stage acts: the request takes the path of one without the parameter"""
        return self.pack() == [0.0, 1.0, 0.0, 0.0]

    def pack(self) -> List[float]:
        """[min_p, typical_p, epsilon_cutoff, eta_cutoff] as gar_sample_ext reads them behind (temperature, top_p, top_k, 0): an
        off stage holds its neutral value 0 / 1 / 0 / 0"""
        typ = 1.0 if self.typical_p is None or self.typical_p >= 1.0 else self.typical_p
        return [self.min_p or 0.0, typ, self.epsilon_cutoff or 0.0, self.eta_cutoff or 0.0]
