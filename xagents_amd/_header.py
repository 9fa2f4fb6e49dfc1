"""Reader of the C ABI header (include/xagents_hip.h): its `#define XA_*` integers, its
`typedef struct` blocks and its prototypes, as the ctypes objects _lib.py binds.

It reads the header's own regular shape, not C: integer `#define`s, one
`typedef struct X { ... } X;` per argument struct (scalar, pointer, earlier-struct and
`[XA_CONST]` array fields), and prototypes that return int, size_t or const char*. Whatever
else it meets raises HeaderError with the header line; it never guesses a type or skips a
declaration.
"""
import ctypes
import re
from collections import namedtuple

Header = namedtuple('Header', 'constants structs signatures')

SCALARS = {
    'int': ctypes.c_int, 'unsigned': ctypes.c_uint, 'short': ctypes.c_short,
    'float': ctypes.c_float, 'double': ctypes.c_double,
    'int64_t': ctypes.c_int64, 'uint64_t': ctypes.c_uint64, 'uint32_t': ctypes.c_uint32,
    'uint8_t': ctypes.c_uint8, 'size_t': ctypes.c_size_t,
}
RETURNS = {'int': ctypes.c_int, 'size_t': ctypes.c_size_t, 'const char*': ctypes.c_char_p}

_COMMENT = re.compile(r'/\*.*?\*/|//[^\n]*', re.S)
# the header's statements; at every position exactly one of them has to match
_CXX_ONLY = re.compile(r'#ifdef __cplusplus\n.*?\n#endif[ \t]*\n', re.S)
_DEFINE = re.compile(r'#define[ \t]+(XA_\w+)[ \t]+(\S[^\n]*)\n')
_DIRECTIVE = re.compile(
    r'#(?:ifndef[ \t]+\w+|endif|include[ \t]+<\w+\.h>|define[ \t]+\w+)[ \t]*\n')
_STRUCT = re.compile(r'typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;')
_PROTOTYPE = re.compile(r'([\w \t*]+?)\s*\b(\w+)\s*\(([^()]*)\)\s*;')
# `[const] word rest` and one declarator `[*[*]] name [[bound]]` of rest
_TYPED = re.compile(r'(?:const\s+)?(\w+)\b\s*(.*)', re.S)
_DECLARATOR = re.compile(r'(\**)\s*(\w+)\s*(?:\[\s*(\w+)\s*\])?')


class HeaderError(ValueError):
    pass


def read_header(text, name='xagents_hip.h'):
    """Header(constants {name: int}, structs {name: ctypes.Structure subclass}, signatures
    {name: (restype, [argtypes])}) of the header `text`, each in declaration order."""
    # comments go first (they hold ';', braces and parentheses); their newlines stay, so a
    # position still tells the header line
    text = _COMMENT.sub(lambda m: '\n' * m.group().count('\n'), text).rstrip() + '\n'
    constants, structs, signatures = {}, {}, {}

    def fail(why, at):
        stmt = ' '.join(text[at:].split('\n' if text[at] == '#' else ';')[0].split())[:120]
        raise HeaderError(f'{name}:{text.count(chr(10), 0, at) + 1}: {why}: {stmt!r}')

    def data_type(word, stars):
        """ctypes type of a field or argument `word stars`; None if the binding has none."""
        if not stars:
            return SCALARS.get(word) or structs.get(word)
        if stars == '*' and (word == 'void' or word in SCALARS or word in structs):
            return ctypes.c_void_p
        return None

    def fields_of(body, start):
        fields = []
        for decl in re.finditer(r'[^;\s][^;]*', body):
            at = start + decl.start()
            typed = _TYPED.fullmatch(decl.group().strip())
            for declarator in typed.group(2).split(',') if typed else [None]:
                d = declarator and _DECLARATOR.fullmatch(declarator.strip())
                if not d:
                    fail('unreadable field', at)
                stars, field, bound = d.groups()
                ctype = data_type(typed.group(1), stars)
                if ctype is None:
                    fail(f'unknown type {typed.group(1) + stars!r} (no scalar of the binding, '
                         f'no struct defined above)', at)
                if bound is not None:
                    if bound not in constants:
                        fail(f'array bound {bound!r} is not a constant defined above', at)
                    ctype = ctype * constants[bound]
                fields.append((field, ctype))
        return fields

    def argtypes_of(params, at):
        args = []
        for param in [] if params.strip() == 'void' else params.split(','):
            typed = _TYPED.fullmatch(param.strip())
            d = typed and _DECLARATOR.fullmatch(typed.group(2))
            if not d or d.group(3):
                fail(f'unreadable argument {param.strip()!r}', at)
            word, stars = typed.group(1), d.group(1)
            if stars == '*' and word in structs:
                ctype = ctypes.POINTER(structs[word])
            elif stars == '**' and word == 'void':
                ctype = ctypes.POINTER(ctypes.c_void_p)
            else:
                ctype = data_type(word, stars)
            if ctype is None or (word in structs and not stars):
                fail(f'unknown argument type {word + stars!r} (no scalar of the binding, no '
                     f'pointer to one or to a struct defined above)', at)
            args.append(ctype)
        return args

    pos = 0
    while pos < len(text):
        if text[pos].isspace():
            pos += 1
            continue
        if m := _DEFINE.match(text, pos):
            try:
                constants[m.group(1)] = int(m.group(2).strip(), 0)
            except ValueError:
                fail('not an integer constant', pos)
        elif m := _STRUCT.match(text, pos):
            if m.group(1) != m.group(3) or m.group(1) in structs:
                fail('struct tag and typedef name differ, or the struct is defined twice', pos)
            structs[m.group(1)] = type(m.group(1), (ctypes.Structure,),
                                       {'_fields_': fields_of(m.group(2), m.start(2))})
        elif m := _PROTOTYPE.match(text, pos):
            restype = RETURNS.get(re.sub(r'\s*\*', '*', ' '.join(m.group(1).split())))
            if restype is None or m.group(2) in signatures:
                fail('unknown return type, or the function is declared twice', pos)
            signatures[m.group(2)] = (restype, argtypes_of(m.group(3), pos))
        elif not (m := _CXX_ONLY.match(text, pos) or _DIRECTIVE.match(text, pos)):
            fail('unreadable declaration', pos)
        pos = m.end()
    return Header(constants, structs, signatures)
