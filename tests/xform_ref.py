"""Pure-Python statement of the deidentify_config semantics (mask / replace / remove / keep per info
type), applied to the oracle's findings: the expected value of the transformation tests.  Written
from the rule table alone; it shares no code with compiler.parse_deidentify."""
import string

CLASSES = {"NUMERIC": string.digits, "ALPHA_UPPER_CASE": string.ascii_uppercase,
           "ALPHA_LOWER_CASE": string.ascii_lowercase, "PUNCTUATION": string.punctuation,
           "WHITESPACE": string.whitespace}


def pick(type_name, config):
    """the primitive_transformation for a type: first entry listing it, else first catch-all, else None"""
    if "deidentify_config" not in config:
        return {"replace_with_info_type_config": {}}
    entries = config["deidentify_config"]["info_type_transformations"]["transformations"]
    for e in entries:
        if type_name in [it["name"] for it in e.get("info_types", [])]:
            return e["primitive_transformation"]
    return next((e["primitive_transformation"] for e in entries if not e.get("info_types")), None)


def mask(piece: bytes, cfg: dict) -> bytes:
    ch = cfg.get("masking_character", "*").encode()
    n = cfg.get("number_to_mask", 0) or len(piece)
    skip = set()
    for ign in cfg.get("characters_to_ignore", []):
        skip |= set(ign.get("characters_to_skip", "")) | set(CLASSES.get(ign.get("common_characters_to_ignore"), ""))
    chars = list(piece.decode("utf-8"))
    order = range(len(chars) - 1, -1, -1) if cfg.get("reverse_order") else range(len(chars))
    out = [c.encode("utf-8") for c in chars]
    for i in order:
        if n > 0 and chars[i] not in skip:
            out[i] = ch * len(out[i])          # every byte of a masked code point
            n -= 1
    return b"".join(out)


def apply_transform(text: bytes, findings, names, config: dict) -> bytes:
    """findings: objects with start / end / type_id, in order, not overlapping"""
    out, pos = [], 0
    for f in findings:
        out.append(text[pos:f.start])
        prim, piece = pick(names[f.type_id], config), text[f.start:f.end]
        if prim is None:
            out.append(piece)
        elif "replace_with_info_type_config" in prim:
            out.append(b"[" + names[f.type_id].encode() + b"]")
        elif "replace_config" in prim:
            out.append(prim["replace_config"]["new_value"]["string_value"].encode("utf-8"))
        elif "character_mask_config" in prim:
            out.append(mask(piece, prim["character_mask_config"]))
        else:
            assert "redact_config" in prim, prim
        pos = f.end
    out.append(text[pos:])
    return b"".join(out)
