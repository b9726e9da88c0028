// json_writer.h — the JSON emitter of the text-returning entries (hfg_profile_summary,
// hfg_debug_plan, hfg_debug_workspace): values in call order, the separators placed here.
#pragma once

#include <cstdio>
#include <initializer_list>
#include <string>

namespace hfg_host {

class JsonWriter {
 public:
  JsonWriter& begin_object() { return item("{", true); }
  JsonWriter& end_object() { return close('}'); }
  JsonWriter& begin_array() { return item("[", true); }
  JsonWriter& end_array() { return close(']'); }
  // the name of the next value inside an object (the value follows without a separator)
  JsonWriter& key(const std::string& k) {
    string(k).s_ += ": ";
    first_ = true;
    return *this;
  }
  JsonWriter& integer(long long v) { return item(std::to_string(v)); }
  // fmt: a printf conversion of one double ("%.6f", "%.6e")
  JsonWriter& real(const char* fmt, double v) {
    char b[64];
    snprintf(b, sizeof(b), fmt, v);
    return item(b);
  }
  JsonWriter& string(const std::string& v) {
    std::string q = "\"";
    for (char c : v) q += (c == '"' || c == '\\') ? std::string("\\") + c : std::string(1, c);
    return item(q + "\"");
  }
  // key and value in one call
  JsonWriter& integer(const std::string& k, long long v) { return key(k).integer(v); }
  JsonWriter& string(const std::string& k, const std::string& v) { return key(k).string(v); }
  template <class Seq>
  JsonWriter& integers(const std::string& k, const Seq& seq) {
    key(k).begin_array();
    for (auto v : seq) integer((long long)v);
    return end_array();
  }
  JsonWriter& integers(const std::string& k, std::initializer_list<long long> seq) {
    return integers<std::initializer_list<long long>>(k, seq);
  }
  const std::string& str() const { return s_; }

 private:
  // opens: no separator in front of the item after this one
  JsonWriter& item(const std::string& text, bool opens = false) {
    if (!first_) s_ += ", ";
    s_ += text;
    first_ = opens;
    return *this;
  }
  JsonWriter& close(char c) {
    s_ += c;
    first_ = false;
    return *this;
  }
  std::string s_;
  bool first_ = true;
};

}  // namespace hfg_host
