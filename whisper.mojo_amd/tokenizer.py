"""Mirror of /root/reference/tokenizer.mojo: id -> text through `vocab.txt` (line index = id,
export_weights.py:134-142).

`decode` reproduces the reference exactly (tokenizer.mojo:15-28): special tokens `<|…|>` are dropped, "Ġ" becomes a
space, the escaped "\\n" a newline — which mangles non-ASCII text, because vocab.txt stores GPT-2 *byte-level* symbols
(e.g. line 50 256 "åľº" is the three bytes e5 9c ba = "场").  `decode_text` adds the correct byte-level un-mapping."""
from __future__ import annotations

from typing import Dict, List, Sequence, Union


def _bytes_to_unicode() -> Dict[int, str]:
    """GPT-2's reversible byte <-> printable-unicode table (the published byte-level BPE alphabet)."""
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(ord("¡"), ord("¬") + 1)) + list(range(ord("®"), ord("ÿ") + 1))
    cs = bs[:]
    n = 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return {b: chr(c) for b, c in zip(bs, cs)}


_UNICODE_TO_BYTE = {c: b for b, c in _bytes_to_unicode().items()}


class Tokenizer:
    """tokenizer.mojo:4-28"""

    def __init__(self, path_or_vocab: Union[str, Sequence[str], Dict[int, str]]):
        if isinstance(path_or_vocab, str):
            with open(path_or_vocab, "r", encoding="utf-8") as f:  # raises like tokenizer.mojo:9
                self.vocab: Union[List[str], Dict[int, str]] = f.read().split("\n")  # tokenizer.mojo:10-13
        else:
            self.vocab = path_or_vocab if isinstance(path_or_vocab, dict) else list(path_or_vocab)

    def _token(self, token_id: int):
        if isinstance(self.vocab, dict):
            return self.vocab.get(token_id)
        return self.vocab[token_id] if 0 <= token_id < len(self.vocab) else None  # tokenizer.mojo:19

    @staticmethod
    def _is_special(token: str) -> bool:
        return token.startswith("<|") and token.endswith("|>")  # tokenizer.mojo:22

    def decode(self, tokens: Sequence[int]) -> str:
        """The reference's rendering, bug for bug (tokenizer.mojo:15-28)."""
        result = ""
        for token_id in tokens:
            token = self._token(int(token_id))
            if token is None or self._is_special(token):
                continue
            result += token.replace("Ġ", " ").replace("\\n", "\n")
        return result

    def decode_text(self, tokens: Sequence[int]) -> str:
        """Correct byte-level BPE decoding: every vocab symbol maps back to one byte; the byte string is UTF-8."""
        data = bytearray()
        for token_id in tokens:
            token = self._token(int(token_id))
            if token is None or self._is_special(token):
                continue
            token = token.replace("\\n", "Ċ")  # export_weights.py:139 escaped the newline symbol's raw form
            for ch in token:
                b = _UNICODE_TO_BYTE.get(ch)
                if b is None:
                    data.extend(ch.encode("utf-8"))
                else:
                    data.append(b)
        return data.decode("utf-8", errors="replace")


# The multilingual checkpoints' language tokens, in id order from <|startoftranscript|> + 1 (openai-whisper's LANGUAGES order;
# the 51865-entry vocabulary has these 99, ids 50259 … 50357).
LANGUAGE_CODES = (
    "en zh de es ru ko fr ja pt tr pl ca nl ar sv it id hi fi vi he uk el ms cs ro da hu ta no th ur hr bg lt la mi ml cy sk te fa lv bn "
    "sr az sl kn et mk br eu is hy ne mn bs kk sq sw gl mr pa si km sn yo so af oc ka be tg sd gu am yi lo uz fo ht ps tk nn mt sa lb my "
    "bo tl mg as tt haw ln ha ba jw su").split()
LANGUAGE_ID0 = 50259


def language_ids(tokenizer: "Tokenizer" = None):
    """The language ids of the multilingual vocabulary, for detect_language: (ids, {id: code}, from_vocab).
    With a tokenizer whose vocabulary holds the `<|xx|>` entries behind <|startoftranscript|>, ids and codes are read from it
    (from_vocab True); without one, or when the vocabulary file lacks those entries, the published range 50259 … 50357 and
    openai-whisper's code order are returned and from_vocab is False."""
    if tokenizer is not None:
        ids, codes = [], {}
        i = LANGUAGE_ID0
        while True:
            tok = tokenizer._token(i)
            if tok is None or not Tokenizer._is_special(tok) or not (2 <= len(tok) - 4 <= 3) or not tok[2:-2].isalpha():
                break
            ids.append(i)
            codes[i] = tok[2:-2]
            i += 1
        if ids and tokenizer._token(LANGUAGE_ID0 - 1) == "<|startoftranscript|>":
            return ids, codes, True
    ids = list(range(LANGUAGE_ID0, LANGUAGE_ID0 + len(LANGUAGE_CODES)))
    return ids, dict(zip(ids, LANGUAGE_CODES)), False


def language_code(token_id: int, tokenizer: "Tokenizer" = None) -> str:
    """<|xx|> id -> "xx"; KeyError for an id that is no language token."""
    return language_ids(tokenizer)[1][int(token_id)]


# ---- word grouping for word-level timestamps --------------------------------------------------------------------------
# A restatement of transformers' tokenization_whisper._collate_word_timestamps for the languages that are split on spaces:
# _split_tokens_on_unicode (a word ends where the ids so far decode to complete UTF-8), _split_tokens_on_spaces, _merge_punctuations.
UNICODE_SPLIT_LANGUAGES = {"chinese", "japanese", "thai", "lao", "myanmar", "cantonese", "zh", "ja", "th", "lo", "my", "yue"}
_PREPEND_PUNCTUATIONS = "\"'“¡¿([{-"
_APPEND_PUNCTUATIONS = "\"'.。,，!！?？:：”)]}、"
_PUNCTUATION = "!\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~"


def _split_on_unicode(tokenizer: "Tokenizer", ids: Sequence[int]):
    full = tokenizer.decode_text(ids)
    bad = "�"
    words, indices, cur, offset = [], [], [], 0
    for k in range(len(ids)):
        cur.append(k)
        text = tokenizer.decode_text([ids[j] for j in cur])
        if bad not in text or offset + text.index(bad) >= len(full) or full[offset + text.index(bad)] == bad:
            words.append(text)
            indices.append(cur)
            cur = []
            offset += len(text)
    return words, indices


def collate_words(tokenizer: "Tokenizer", ids: Sequence[int], pairs: Sequence[Sequence[float]], language: str = None,
                  eos_token_id: int = 50257) -> List[dict]:
    """ids of one segment and their (start, end) pairs -> [{"text": word, "timestamp": (start of its first id, end of its last)}],
    as HF's _collate_word_timestamps groups them: a new word at an id that decodes with a leading space, at a punctuation mark and
    at an id >= eos_token_id; then the prepended / appended punctuation marks join their neighbours.  NotImplementedError for the
    languages HF splits on unicode points instead."""
    if language is not None and language.lower() in UNICODE_SPLIT_LANGUAGES:
        raise NotImplementedError(f"word grouping for {language!r} (split on unicode points) is not implemented")
    ids = [int(t) for t in ids]
    words, indices = [], []
    for sub, idx in zip(*_split_on_unicode(tokenizer, ids)):
        special = ids[idx[0]] >= eos_token_id
        if special or sub.startswith(" ") or sub.strip() in _PUNCTUATION or not words:
            words.append(sub)
            indices.append(list(idx))
        else:
            words[-1] += sub
            indices[-1].extend(idx)
    i, j = len(words) - 2, len(words) - 1
    while i >= 0:  # prepended marks go to the word that follows
        if words[i].startswith(" ") and words[i].strip() in _PREPEND_PUNCTUATIONS:
            words[j] = words[i] + words[j]
            indices[j] = indices[i] + indices[j]
            words[i], indices[i] = "", []
        else:
            j = i
        i -= 1
    i, j = 0, 1
    while j < len(words):  # appended marks go to the word before
        if not words[i].endswith(" ") and words[j] in _APPEND_PUNCTUATIONS:
            words[i] += words[j]
            indices[i] += indices[j]
            words[j], indices[j] = "", []
        else:
            i = j
        j += 1
    words = [w for w in words if w]      # (HF filters the two lists separately; so does this)
    indices = [x for x in indices if x]
    return [{"text": w, "timestamp": (pairs[x[0]][0], pairs[x[-1]][1])} for w, x in zip(words, indices)]
