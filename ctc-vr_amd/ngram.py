"""Back-off n-gram language model for shallow fusion in the CTC and the transducer prefix beam search (rnnt_ngram_set; semantics in
include/rnnt_hip.h).  Host data only: the library builds the automaton."""
import math
from typing import Dict, List, Sequence, Tuple

_LN10 = math.log(10.0)


class NgramLM:
    """ngrams [(tokens, logp, bow), ...]: model token ids (BOS = vocab_size first, EOS = vocab_size + 1 last, never the blank),
    natural-log probability and back-off weight; every n-gram's prefix is listed before it (orders ascending does that).
    lm_weight scales the model's log-probabilities, length_bonus is added per emitted token, unk_logp is the log-probability of a
    token without a unigram."""

    def __init__(self, ngrams: Sequence[Tuple[Sequence[int], float, float]], lm_weight: float = 0.5, length_bonus: float = 0.0,
                 unk_logp: float = math.log(1e-10)):
        self.ngrams: List[Tuple[Tuple[int, ...], float, float]] = [(tuple(int(t) for t in g[0]), float(g[1]), float(g[2])) for g in ngrams]
        self.lm_weight, self.length_bonus, self.unk_logp = float(lm_weight), float(length_bonus), float(unk_logp)

    @classmethod
    def from_arpa(cls, text: str, token_to_id: Dict[str, int], bos: str = "<s>", eos: str = "</s>", **kw) -> "NgramLM":
        """The model of an ARPA file's text.  token_to_id maps the words to model ids and must hold `vocab_size` under the key bos and
        `vocab_size + 1` under eos for those two to be kept.  log10 values become natural logs; a missing back-off weight is 0; orders
        are emitted ascending, in file order inside an order; an n-gram that holds a word outside token_to_id is dropped, and so is
        every n-gram whose prefix was dropped or is missing."""
        by_order: Dict[int, List[Tuple[Tuple[int, ...], float, float]]] = {}
        order = 0
        for line in text.splitlines():
            line = line.strip()
            if not line or line == "\\data\\" or line.startswith("ngram "):
                continue
            if line == "\\end\\":
                break
            if line.startswith("\\") and line.endswith("-grams:"):
                order = int(line[1:-len("-grams:")])
                by_order.setdefault(order, [])
                continue
            if order == 0:
                continue
            f = line.split()
            if len(f) not in (order + 1, order + 2):
                raise ValueError(f"ARPA: {order}-gram line with {len(f)} fields: {line!r}")
            words = f[1:1 + order]
            if any(w not in token_to_id for w in words):
                continue
            bow = float(f[order + 1]) * _LN10 if len(f) == order + 2 else 0.0
            by_order[order].append((tuple(int(token_to_id[w]) for w in words), float(f[0]) * _LN10, bow))
        seen, grams = {()}, []
        for order in sorted(by_order):
            for toks, logp, bow in by_order[order]:
                if toks[:-1] in seen and toks not in seen:
                    seen.add(toks)
                    grams.append((toks, logp, bow))
        return cls(grams, **kw)
