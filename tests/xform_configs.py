"""The deidentify_config blocks the transformation tests use, and the shipped config with only that
block replaced (the oracle ignores the block, so its findings stay the reference)."""
import json
import os

from conftest import pkg


def _mask(**kw):
    return {"character_mask_config": kw}


def _types(*names):
    return [{"name": n} for n in names]


CARD_MASK = _mask(masking_character="#", number_to_mask=12, characters_to_ignore=[{"characters_to_skip": " -"}])

# A: no catch-all -- unlisted types keep their bytes
A = [
    {"info_types": _types("CREDIT_CARD_NUMBER"), "primitive_transformation": CARD_MASK},
    {"info_types": _types("US_SOCIAL_SECURITY_NUMBER"),
     "primitive_transformation": _mask(masking_character="*", number_to_mask=4, reverse_order=True)},
    {"info_types": _types("EMAIL_ADDRESS"),
     "primitive_transformation": {"replace_config": {"new_value": {"string_value": "<email>"}}}},
    {"info_types": _types("SOCIAL_HANDLE"), "primitive_transformation": {"redact_config": {}}},
    {"info_types": _types("PHONE_NUMBER"),
     "primitive_transformation": _mask(masking_character="*",
                                       characters_to_ignore=[{"common_characters_to_ignore": "PUNCTUATION"}])},
]
# B: one catch-all mask that keeps punctuation and white space: every row keeps its length
B = [{"primitive_transformation": _mask(masking_character="*", characters_to_ignore=[
    {"common_characters_to_ignore": "PUNCTUATION"}, {"common_characters_to_ignore": "WHITESPACE"}])}]
# C: everything removed, except the card number masked as in A
C = [{"info_types": _types("CREDIT_CARD_NUMBER"), "primitive_transformation": CARD_MASK},
     {"primitive_transformation": {"redact_config": {}}}]


# known answers under A (shipped rules, no context): literal, not computed
KNOWN_A = [
    (b"my ssn is 536-22-1234@johnny thanks", b"my ssn is 536-22-**** thanks"),          # findings touch at 21
    (b"card number 4111 1111 1111 1111 ok", b"card number #### #### #### 1111 ok"),
    (b"card number 4111-1111-1111-1111", b"card number ####-####-####-1111"),
    (b"reach me at jane.doe@corp.example.org or 212-555-0187", b"reach me at <email> or ***-***-****"),
    (b"@johnny", b""),
    (b"A1234567@bob_1", b"A1234567"),                      # ALIEN_REGISTRATION_NUMBER is unlisted: kept
    (b"ip address 10.20.30.40", b"ip address 10.20.30.40"),
]
# external candidate: PERSON_NAME at likelihood 4 over "José Núñez" (bytes 5..17 of the row)
EXT_TEXT = "I am José Núñez ok".encode()
EXT_SPAN = (5, 5 + len("José Núñez".encode()))
KNOWN_EXT = [
    (_mask(masking_character="*", number_to_mask=2), "I am **sé Núñez ok".encode()),
    (_mask(masking_character="*", number_to_mask=3, reverse_order=True,
           characters_to_ignore=[{"characters_to_skip": " "}]), "I am José Nú**** ok".encode()),
]

# A masked finding of several 16-byte windows of the mask walk (windows count from the finding's first
# byte, or from its last when reverse_order): one PERSON_NAME external candidate of 68 bytes, 1- to 4-byte
# code points, spaces and '-'.  A code point straddles the window edges at bytes 16 and 32 and, from the end,
# at 52, 36 and 20.  The external-candidate entry points do not limit a candidate's length.
LONG_NAME = "Zoë-Renée 李小龍 Ñandú 𝒜𝓁𝒾 Łukasz-Ødegård 𐍈bé".encode()
LONG_PREFIX = b"it is me, I am "                 # its last 0 .. 15 bytes precede the name
LONG_SUFFIX = b" ok, that is all there is to it"
LONG_MASKS = {
    "forward_all": _mask(masking_character="*"),
    "forward_18": _mask(masking_character="#", number_to_mask=18),                # ends at byte 27: second window
    "reverse_all": _mask(masking_character="*", reverse_order=True),
    "reverse_21": _mask(masking_character="*", number_to_mask=21, reverse_order=True,     # ends at byte 26: third
                        characters_to_ignore=[{"characters_to_skip": " -"}]),
}


def long_rows():
    """16 rows of 96 bytes -> (texts, [(start, end)] of the name in each): 0 .. 15 bytes before the name, so
    that in a batch packed back to back it starts at each of the 16 byte offsets modulo 16 once"""
    texts, spans = [], []
    for a in range(16):
        row = LONG_PREFIX[len(LONG_PREFIX) - a:] + LONG_NAME
        texts.append(row + LONG_SUFFIX[:96 - len(row)])
        spans.append((a, a + len(LONG_NAME)))
    return texts, spans


def shipped() -> dict:
    with open(os.path.join(pkg("compiler").RULES_DIR, "dlp_config.json")) as f:
        return json.load(f)


def with_block(transformations) -> dict:
    """the shipped config with deidentify_config replaced; None = the shipped block"""
    cfg = shipped()
    if transformations is not None:
        cfg["deidentify_config"] = {"info_type_transformations": {"transformations": transformations}}
    return cfg


def write(tmp_dir, name: str, cfg: dict) -> str:
    path = os.path.join(str(tmp_dir), name + ".json")
    with open(path, "w") as f:
        json.dump(cfg, f)
    return path
