// The JSON reader of `katago analysis` (cli_analysis.cpp): exactly what its query lines need
// -- one flat object per line whose values are strings, integers or arrays of strings -- and
// nothing else.  Anything outside that (nesting, numbers with a fraction, literals, bad UTF-8,
// control characters, over-long input) is rejected with a message.  A caller's Schema may name
// keys that also take a true / false literal or an array of flat objects (the allowMoves /
// avoidMoves shape); the objects inside such an array take the flat values only, so the depth
// is two at most and no input can exhaust the stack.  Host-only and header-only; compiles on
// its own.
#pragma once
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

namespace kcjson {

constexpr size_t MAX_LINE = 1 << 16;   // bytes of one query line
constexpr size_t MAX_FIELDS = 64;      // keys of the object
constexpr size_t MAX_ITEMS = 1024;     // elements of one array
constexpr size_t MAX_STRING = 4096;    // bytes of one string

struct Object;
struct Value {
  // BOOL and OBJECTS only under the keys a Schema names (parseLine)
  enum Kind { STRING, INT, STRINGS, BOOL, OBJECTS } kind = STRING;
  std::string s;
  long long i = 0;  // BOOL: 0 / 1
  std::vector<std::string> a;
  std::vector<Object> objs;  // OBJECTS: flat objects (strings, integers, arrays of strings)
};

// The keys of the top-level object that take more than the flat values: a true / false literal
// (includePolicy) or an array of flat objects (allowMoves, avoidMoves).  Null-terminated lists.
struct Schema {
  const char* const* boolKeys = nullptr;
  const char* const* objectArrayKeys = nullptr;
  static bool has(const char* const* keys, const std::string& k) {
    for(; keys && *keys; keys++)
      if(k == *keys)
        return true;
    return false;
  }
};

struct Object {
  std::vector<std::pair<std::string, Value>> fields;
  const Value* find(const std::string& key) const {
    for(const auto& f : fields)
      if(f.first == key)
        return &f.second;
    return nullptr;
  }
};

namespace detail {

struct Cursor {
  const std::string& s;
  size_t p = 0;
  std::string err;
  explicit Cursor(const std::string& str) : s(str) {}
  bool fail(const std::string& m) {
    if(err.empty())
      err = m + " at byte " + std::to_string(p);
    return false;
  }
  void ws() {
    while(p < s.size() && (s[p] == ' ' || s[p] == '\t' || s[p] == '\r' || s[p] == '\n'))
      p++;
  }
  bool eat(char c) {
    ws();
    if(p < s.size() && s[p] == c) {
      p++;
      return true;
    }
    return false;
  }
};

inline void appendUtf8(std::string& out, uint32_t cp) {
  if(cp < 0x80) {
    out += (char)cp;
  } else if(cp < 0x800) {
    out += (char)(0xC0 | (cp >> 6));
    out += (char)(0x80 | (cp & 0x3F));
  } else if(cp < 0x10000) {
    out += (char)(0xE0 | (cp >> 12));
    out += (char)(0x80 | ((cp >> 6) & 0x3F));
    out += (char)(0x80 | (cp & 0x3F));
  } else {
    out += (char)(0xF0 | (cp >> 18));
    out += (char)(0x80 | ((cp >> 12) & 0x3F));
    out += (char)(0x80 | ((cp >> 6) & 0x3F));
    out += (char)(0x80 | (cp & 0x3F));
  }
}

inline bool hex4(Cursor& c, uint32_t& v) {
  if(c.p + 4 > c.s.size())
    return c.fail("truncated \\u escape");
  v = 0;
  for(int k = 0; k < 4; k++) {
    const char ch = c.s[c.p + k];
    uint32_t d;
    if(ch >= '0' && ch <= '9')
      d = (uint32_t)(ch - '0');
    else if(ch >= 'a' && ch <= 'f')
      d = (uint32_t)(ch - 'a' + 10);
    else if(ch >= 'A' && ch <= 'F')
      d = (uint32_t)(ch - 'A' + 10);
    else
      return c.fail("bad \\u escape");
    v = v * 16 + d;
  }
  c.p += 4;
  return true;
}

// One multi-byte UTF-8 sequence starting at c.p (lead byte >= 0x80), copied to out.
inline bool utf8Sequence(Cursor& c, std::string& out) {
  const unsigned char b0 = (unsigned char)c.s[c.p];
  int n;
  uint32_t cp;
  if(b0 >= 0xC2 && b0 <= 0xDF) {
    n = 1;
    cp = b0 & 0x1F;
  } else if(b0 >= 0xE0 && b0 <= 0xEF) {
    n = 2;
    cp = b0 & 0x0F;
  } else if(b0 >= 0xF0 && b0 <= 0xF4) {
    n = 3;
    cp = b0 & 0x07;
  } else {
    return c.fail("invalid UTF-8");
  }
  if(c.p + (size_t)n >= c.s.size())
    return c.fail("truncated UTF-8");
  for(int k = 1; k <= n; k++) {
    const unsigned char b = (unsigned char)c.s[c.p + k];
    if((b & 0xC0) != 0x80)
      return c.fail("invalid UTF-8");
    cp = (cp << 6) | (b & 0x3F);
  }
  // overlong forms, surrogates and code points past U+10FFFF
  if((n == 2 && cp < 0x800) || (n == 3 && cp < 0x10000) || cp > 0x10FFFF || (cp >= 0xD800 && cp <= 0xDFFF))
    return c.fail("invalid UTF-8");
  out.append(c.s, c.p, (size_t)n + 1);
  c.p += (size_t)n + 1;
  return true;
}

inline bool parseString(Cursor& c, std::string& out) {
  c.ws();
  if(c.p >= c.s.size() || c.s[c.p] != '"')
    return c.fail("expected a string");
  c.p++;
  out.clear();
  for(;;) {
    if(c.p >= c.s.size())
      return c.fail("unterminated string");
    if(out.size() > MAX_STRING)
      return c.fail("string too long");
    const unsigned char ch = (unsigned char)c.s[c.p];
    if(ch == '"') {
      c.p++;
      return true;
    }
    if(ch < 0x20)
      return c.fail("control character in string");
    if(ch >= 0x80) {
      if(!utf8Sequence(c, out))
        return false;
      continue;
    }
    if(ch != '\\') {
      out += (char)ch;
      c.p++;
      continue;
    }
    if(c.p + 1 >= c.s.size())
      return c.fail("unterminated string");
    const char e = c.s[c.p + 1];
    c.p += 2;
    switch(e) {
      case '"': out += '"'; break;
      case '\\': out += '\\'; break;
      case '/': out += '/'; break;
      case 'b': out += '\b'; break;
      case 'f': out += '\f'; break;
      case 'n': out += '\n'; break;
      case 'r': out += '\r'; break;
      case 't': out += '\t'; break;
      case 'u': {
        uint32_t cp;
        if(!hex4(c, cp))
          return false;
        if(cp >= 0xDC00 && cp <= 0xDFFF)
          return c.fail("lone surrogate");
        if(cp >= 0xD800 && cp <= 0xDBFF) {
          uint32_t lo;
          if(c.p + 2 > c.s.size() || c.s[c.p] != '\\' || c.s[c.p + 1] != 'u')
            return c.fail("lone surrogate");
          c.p += 2;
          if(!hex4(c, lo))
            return false;
          if(lo < 0xDC00 || lo > 0xDFFF)
            return c.fail("lone surrogate");
          cp = 0x10000 + ((cp - 0xD800) << 10) + (lo - 0xDC00);
        }
        appendUtf8(out, cp);
        break;
      }
      default: return c.fail("bad escape");
    }
  }
}

inline bool parseInt(Cursor& c, long long& out) {
  c.ws();
  const size_t start = c.p;
  bool neg = false;
  if(c.p < c.s.size() && c.s[c.p] == '-') {
    neg = true;
    c.p++;
  }
  if(c.p >= c.s.size() || c.s[c.p] < '0' || c.s[c.p] > '9')
    return c.fail("expected an integer");
  if(c.s[c.p] == '0' && c.p + 1 < c.s.size() && c.s[c.p + 1] >= '0' && c.s[c.p + 1] <= '9')
    return c.fail("leading zero");
  unsigned long long v = 0;
  while(c.p < c.s.size() && c.s[c.p] >= '0' && c.s[c.p] <= '9') {
    if(c.p - start > 18)  // 18 digits fit in a signed 64-bit integer
      return c.fail("integer out of range");
    v = v * 10 + (unsigned long long)(c.s[c.p] - '0');
    c.p++;
  }
  if(c.p < c.s.size() && (c.s[c.p] == '.' || c.s[c.p] == 'e' || c.s[c.p] == 'E'))
    return c.fail("only integers are supported");
  out = neg ? -(long long)v : (long long)v;
  return true;
}

inline bool parseFields(Cursor& c, Object& out, const Schema* schema);

// key / schema: the value's key in the top-level object (schema null: inside an array's
// object, where only the flat values are taken -- the depth is bounded by that).
inline bool parseValue(Cursor& c, Value& v, const Schema* schema = nullptr, const std::string& key = std::string()) {
  c.ws();
  if(c.p >= c.s.size())
    return c.fail("truncated line");
  const char ch = c.s[c.p];
  if(schema && Schema::has(schema->boolKeys, key) && (ch == 't' || ch == 'f')) {
    const char* word = ch == 't' ? "true" : "false";
    const size_t n = ch == 't' ? 4 : 5;
    if(c.s.compare(c.p, n, word) != 0)
      return c.fail("expected true or false");
    c.p += n;
    v.kind = Value::BOOL;
    v.i = ch == 't' ? 1 : 0;
    return true;
  }
  if(schema && Schema::has(schema->objectArrayKeys, key) && ch == '[') {
    c.p++;
    v.kind = Value::OBJECTS;
    v.objs.clear();
    if(c.eat(']'))
      return true;
    for(;;) {
      if(v.objs.size() >= MAX_ITEMS)
        return c.fail("array too long");
      if(!c.eat('{'))
        return c.fail(c.p >= c.s.size() ? "truncated line" : "expected an object");
      v.objs.emplace_back();
      if(!parseFields(c, v.objs.back(), nullptr))
        return false;
      if(c.eat(','))
        continue;
      if(c.eat(']'))
        return true;
      return c.fail(c.p >= c.s.size() ? "truncated line" : "expected ',' or ']'");
    }
  }
  if(ch == '"') {
    v.kind = Value::STRING;
    return parseString(c, v.s);
  }
  if(ch == '-' || (ch >= '0' && ch <= '9')) {
    v.kind = Value::INT;
    return parseInt(c, v.i);
  }
  if(ch == '{')
    return c.fail("nested objects are not supported");
  if(ch != '[')
    return c.fail("expected a string, an integer or an array of strings");
  c.p++;
  v.kind = Value::STRINGS;
  v.a.clear();
  if(c.eat(']'))
    return true;
  for(;;) {
    c.ws();
    if(c.p < c.s.size() && (c.s[c.p] == '[' || c.s[c.p] == '{'))
      return c.fail("nested arrays are not supported");
    if(v.a.size() >= MAX_ITEMS)
      return c.fail("array too long");
    std::string item;
    if(!parseString(c, item))
      return false;
    v.a.push_back(std::move(item));
    if(c.eat(','))
      continue;
    if(c.eat(']'))
      return true;
    return c.fail(c.p >= c.s.size() ? "truncated line" : "expected ',' or ']'");
  }
}

// An object's fields up to and including its '}' (the '{' is consumed).
inline bool parseFields(Cursor& c, Object& out, const Schema* schema) {
  if(c.eat('}'))
    return true;
  for(;;) {
    if(out.fields.size() >= MAX_FIELDS)
      return c.fail("too many keys");
    std::string key;
    if(!parseString(c, key))
      return false;
    if(out.find(key))
      return c.fail("duplicate key '" + key + "'");
    if(!c.eat(':'))
      return c.fail(c.p >= c.s.size() ? "truncated line" : "expected ':'");
    Value v;
    if(!parseValue(c, v, schema, key))
      return false;
    out.fields.emplace_back(std::move(key), std::move(v));
    if(c.eat(','))
      continue;
    if(c.eat('}'))
      return true;
    return c.fail(c.p >= c.s.size() ? "truncated line" : "expected ',' or '}'");
  }
}

}  // namespace detail

// Parses one line into out; on failure returns false with a message in err.  schema (null:
// flat values only): the keys that take a literal or an array of flat objects.
inline bool parseLine(const std::string& line, Object& out, std::string& err, const Schema* schema = nullptr) {
  out.fields.clear();
  if(line.size() > MAX_LINE) {
    err = "line longer than " + std::to_string(MAX_LINE) + " bytes";
    return false;
  }
  detail::Cursor c(line);
  auto bad = [&]() {
    err = c.err;
    return false;
  };
  if(!c.eat('{')) {
    c.fail(c.p >= line.size() ? "empty line" : "expected '{'");
    return bad();
  }
  if(!detail::parseFields(c, out, schema))
    return bad();
  c.ws();
  if(c.p != line.size()) {
    c.fail("text after the object");
    return bad();
  }
  return true;
}

// s as a JSON string literal (the output side).
inline std::string quote(const std::string& s) {
  std::string o = "\"";
  for(const unsigned char ch : s) {
    if(ch == '"' || ch == '\\') {
      o += '\\';
      o += (char)ch;
    } else if(ch < 0x20) {
      const char* hex = "0123456789abcdef";
      o += "\\u00";
      o += hex[ch >> 4];
      o += hex[ch & 15];
    } else {
      o += (char)ch;
    }
  }
  return o + "\"";
}

}  // namespace kcjson
